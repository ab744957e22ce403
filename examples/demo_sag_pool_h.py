# coding=utf-8
"""Hierarchical SAGPool graph classification — the MI355X counterpart of the reference's demo/demo_sag_pool_h.py.

Same model: 3 x (GCN(128, relu) -> SAGPool(GCN(1), ratio 0.5, tanh)), a mean || max readout after every level, the three
readouts summed, then Dense(128, relu) -> Dropout(0.5) -> Dense(64, relu) -> Dense(num_classes); Adam(lr 5e-4), batches of
512 graphs.  NCI1 needs a download (there is no network here), so the data is a seeded NCI1-shaped stand-in: graphs of
10-50 nodes with 37 one-hot node labels; a graph is of class 1 when it holds a planted motif — a 6-cycle of nodes with
label 5 — and of class 0 when its label-5 nodes are scattered (same label counts, no cycle).

    python examples/demo_sag_pool_h.py [--epochs 30] [--graphs 4000] [--static] [--capture]

Every coarsening step runs on the induced-subgraph kernels; each pooled edge list carries a CSR plan derived from its
parent's, so the GCNs of the next level do not sort.

--static trains on fixed-shape batches instead: a GraphStore holds the training graphs on the device, a StaticLoader hands on
graph ids from a device cursor, collate_static assembles them at capacities the host computed once, and every level is
SAGPool.pool_static (a static batch in, a static batch out) with the readouts the batches carry — no host read anywhere in the
step.  --capture (implies --static) records ids -> batch -> three levels -> loss -> backward -> Adam once with
tfg.CapturedTrainStep and replays it.  Without either flag the program is what it was.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd import autograd as AG   # noqa: E402

NUM_LABELS = 37
MOTIF_LABEL = 5
MOTIF_SIZE = 6


class Dataset(object):
    def __init__(self, graphs, labels):
        self.graphs = graphs           # list of (node_labels int [n], edge_index int32 [2, e])
        self.labels = labels
        self.num_features = NUM_LABELS
        self.num_classes = 2


def _random_graph(rng, n):
    """A connected molecule-like skeleton: a random tree plus a few extra bonds; undirected (both directions)."""
    parent = np.array([rng.integers(0, i) for i in range(1, n)])
    a = np.concatenate([np.arange(1, n), rng.integers(0, n, n // 8)])
    b = np.concatenate([parent, rng.integers(0, n, n // 8)])
    keep = a != b
    return a[keep], b[keep]


def make_dataset(num_graphs=4000, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs, labels = [], []
    for i in range(num_graphs):
        n = int(rng.integers(10, 51))
        y = i % 2
        node_labels = rng.integers(0, NUM_LABELS, n)
        node_labels[node_labels == MOTIF_LABEL] = MOTIF_LABEL + 1
        a, b = _random_graph(rng, n)
        motif = rng.choice(n, MOTIF_SIZE, replace=False)
        node_labels[motif] = MOTIF_LABEL
        if y == 1:       # close the label-5 nodes into a cycle
            a = np.concatenate([a, motif])
            b = np.concatenate([b, np.roll(motif, 1)])
        ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int32)
        graphs.append((node_labels, ei))
        labels.append(y)
    order = rng.permutation(num_graphs)
    return Dataset([graphs[i] for i in order], np.asarray(labels, dtype=np.int64)[order])


def make_batch(data, indices, dev=None):
    """BatchGraph.from_graphs: nodes concatenated, edge ids offset, node_graph_index = position in the batch."""
    dev = dev or torch.device("cuda")
    xs, eis, gids, off = [], [], [], 0
    for j, i in enumerate(indices):
        node_labels, ei = data.graphs[i]
        n = node_labels.size
        x = np.zeros((n, NUM_LABELS), dtype=np.float32)
        x[np.arange(n), node_labels] = 1.0
        xs.append(x)
        eis.append(ei + off)
        gids.append(np.full(n, j, dtype=np.int32))
        off += n
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return (to(np.concatenate(xs)), to(np.concatenate(eis, axis=1)), to(np.concatenate(gids)),
            to(data.labels[np.asarray(indices)]), len(indices))


def _glorot(gen, a, b, dev):
    lim = math.sqrt(6.0 / (a + b))
    return ((torch.rand((a, b), generator=gen) * 2.0 - 1.0) * lim).to(dev).requires_grad_(True)


class SAGPoolHModel(object):
    def __init__(self, num_features, num_classes, seed=0):
        dev = torch.device("cuda")
        self.gcns, self.sag_pools = [], []
        for level in range(3):
            self.gcns.append(tfg.layers.GCN(128, activation=tfg.relu, seed=seed + 2 * level))
            self.sag_pools.append(tfg.layers.SAGPool(score_gnn=tfg.layers.GCN(1, seed=seed + 2 * level + 1), ratio=0.5,
                                                     score_activation=torch.tanh))
            self.gcns[-1]._maybe_build([torch.empty(1, num_features if level == 0 else 128)])
            self.sag_pools[-1].score_gnn._maybe_build([torch.empty(1, 128)])
        for layer in self.gcns + self.sag_pools:
            layer.trainable(True)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.mlp = [(_glorot(gen, 256, 128, dev), torch.zeros(128, device=dev, requires_grad=True)),
                    (_glorot(gen, 128, 64, dev), torch.zeros(64, device=dev, requires_grad=True)),
                    (_glorot(gen, 64, num_classes, dev), torch.zeros(num_classes, device=dev, requires_grad=True))]

    def parameters(self):
        ps = []
        for layer in self.gcns + self.sag_pools:
            ps += layer.parameters()
        for k, b in self.mlp:
            ps += [k, b]
        return ps

    def __call__(self, inputs, training=False):
        x, edge_index, node_graph_index, num_graphs = inputs
        edge_weight = None
        h = x
        outputs = []
        for gcn, sag_pool in zip(self.gcns, self.sag_pools):
            h = gcn([h, edge_index, edge_weight], training=training)
            h, edge_index, edge_weight, node_graph_index = sag_pool([h, edge_index, edge_weight, node_graph_index],
                                                                    training=training)
            outputs.append(torch.cat([tfg.nn.mean_pool(h, node_graph_index, num_graphs),
                                      tfg.nn.max_pool(h, node_graph_index, num_graphs)], dim=-1))
        h = outputs[0] + outputs[1] + outputs[2]
        (k0, b0), (k1, b1), (k2, b2) = self.mlp
        h = AG.linear(h, k0, b0, tfg._lib.ACT_RELU)
        if training:
            h = torch.nn.functional.dropout(h, 0.5, training=True)
        h = AG.linear(h, k1, b1, tfg._lib.ACT_RELU)
        return AG.linear(h, k2, b2)


def static_logits(model, batch, training=False, levels=None):
    """The model on a StaticBatchGraph: one row of logits per SLOT (dead slots: the biases alone).  Level by level the pooled
    batch replaces its parent (and is appended to `levels` when a list is given); mean || max readouts through the graph plan
    each batch carries."""
    h, outputs = batch.x, []
    for gcn, sag_pool in zip(model.gcns, model.sag_pools):
        h = gcn([h, batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
        batch = sag_pool.pool_static(h, batch, training=training)
        h = batch.x
        if levels is not None:
            levels.append(batch)
        outputs.append(torch.cat([batch.readout(h, "mean"), batch.readout(h, "max")], dim=-1))
    h = outputs[0] + outputs[1] + outputs[2]
    (k0, b0), (k1, b1), (k2, b2) = model.mlp
    h = AG.linear(h, k0, b0, tfg._lib.ACT_RELU)
    if training:
        h = torch.nn.functional.dropout(h, 0.5, training=True)
    h = AG.linear(h, k1, b1, tfg._lib.ACT_RELU)
    return AG.linear(h, k2, b2)


def static_loss(model, batch, training=True):
    """Mean cross-entropy over the LIVE slots (a dead slot holds graph 0's label: torch.where on graph_mask)."""
    per_slot = torch.nn.functional.cross_entropy(static_logits(model, batch, training=training), batch.y.reshape(-1),
                                                 reduction="none")
    zero = torch.zeros((), dtype=per_slot.dtype, device=per_slot.device)
    return torch.where(batch.graph_mask, per_slot, zero).sum() / batch.counts[0].clamp(min=1).to(per_slot.dtype)


def graph_store(data, indices):
    graphs = []
    for i in indices:
        node_labels, ei = data.graphs[i]
        x = np.zeros((node_labels.size, NUM_LABELS), dtype=np.float32)
        x[np.arange(node_labels.size), node_labels] = 1.0
        graphs.append(tfg.Graph(x, ei, y=data.labels[i:i + 1]))
    return tfg.data.GraphStore(graphs)


def make_static_step(model, store, loader, capacities, opt, capture, loss=None):
    """step() -> the loss (a device scalar) of one training step on the loader's next batch.  capture=True records the step once
    with tfg.CapturedTrainStep (opt must be capturable) and replays it.  loss(model, batch): static_loss when None (another
    example's model brings its own: demo_sort_pool.py)."""
    loss = static_loss if loss is None else loss

    def loss_fn():
        return loss(model, store.collate_static(loader.next_ids(), capacities))

    if not capture:
        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn()
            loss.backward()
            opt.step()
            return loss
        return step
    cursor, rng_state = loader.cursor.clone(), torch.cuda.get_rng_state()
    step = tfg.CapturedTrainStep(loss_fn, opt)
    # the warm-up steps and the capture advanced the loader's cursor and the dropout generator; the constructor rolled the
    # weights and the optimizer state back, these two are rolled back here: replay k then draws the batch AND the dropout
    # masks of eager step k, so a --capture run trains exactly as a --static run does
    loader.cursor.copy_(cursor)
    torch.cuda.set_rng_state(rng_state)
    return step


def train_static(model, data, train_idx, test_batches, args):
    """The --static / --capture route: the epochs of main() over fixed-shape batches."""
    store = graph_store(data, train_idx)
    loader = store.static_loader(args.batch_size, shuffle=True, seed=args.seed + 1)
    cap = store.static_capacities(args.batch_size)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, capturable=args.capture)
    step = make_static_step(model, store, loader, cap, opt, args.capture)
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


def evaluate(model, batches):
    correct = total = 0
    with torch.no_grad():
        for x, ei, gid, y, num_graphs in batches:
            pred = model([x, ei, gid, num_graphs]).argmax(-1)
            correct += int((pred == y).sum().item())
            total += int(y.shape[0])
    return correct / max(total, 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--static", action="store_true", help="fixed-shape batches: collate_static and SAGPool.pool_static")
    p.add_argument("--capture", action="store_true", help="replay the whole step from one hipGraph (implies --static)")
    args = p.parse_args()
    torch.manual_seed(args.seed)
    data = make_dataset(args.graphs, args.seed)
    n_test = len(data.graphs) // 10
    train_idx = np.arange(n_test, len(data.graphs))
    test_batches = [make_batch(data, list(range(i, min(i + args.batch_size, n_test)))) for i in range(0, n_test, args.batch_size)]
    model = SAGPoolHModel(data.num_features, data.num_classes, seed=args.seed)
    if args.static or args.capture:
        return train_static(model, data, train_idx, test_batches, args)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    train_batches = None
    for epoch in range(args.epochs):
        order = rng.permutation(train_idx)
        train_batches = [make_batch(data, list(order[i:i + args.batch_size])) for i in range(0, order.size, args.batch_size)]
        t0 = time.perf_counter()
        losses = [train_step(model, opt, b) for b in train_batches]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / len(train_batches)
        print("epoch {:3d}  loss {:.4f}  test accuracy {:.4f}  ({:.1f} ms / step)".format(
            epoch, float(np.mean(losses)), evaluate(model, test_batches), ms), flush=True)


if __name__ == "__main__":
    main()
