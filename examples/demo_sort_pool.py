# coding=utf-8
"""DGCNN graph classification with SortPool — the MI355X counterpart of the reference's demo/demo_sort_pool.py.

Same model: 3 x GCN(128, relu) -> SortPool(k = 30) -> convert_x_to_3d -> Conv1D(128, 5, relu) -> Flatten -> Dense(128, relu) ->
Dropout(0.5) -> Dense(num_classes); Adam(lr 5e-4), batches of 512 graphs, on the seeded NCI1-shaped stand-in of
demo_sag_pool_h.py (NCI1 needs a download).

    python examples/demo_sort_pool.py [--epochs 30] [--graphs 4000] [--fused] [--static] [--capture]

By default the readout is written as the reference writes it: the SortPool layer (the pooled graph with its induced edge list,
which the model never looks at), then tfg.utils.convert_x_to_3d.  --fused takes SortPool.pool_3d instead: node rows straight to
[G, k, F] in one launch, the same bits.  --static trains on fixed-shape batches (GraphStore.collate_static, SortPool.pool_static:
no host read anywhere in the step), and --capture (implies --static) records ids -> batch -> model -> loss -> backward -> Adam
once with tfg.CapturedTrainStep and replays it.

The Conv1D is a window view of the [G, 30, 128] tensor and ONE dense product on the library's GEMM ([G * 26, 5 * 128] x
[5 * 128, 128]), so no library algorithm search sits inside a capture.
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
from demo_sag_pool_h import make_dataset, make_batch, graph_store, make_static_step, _glorot   # noqa: E402

K = 30
UNITS = 128
WINDOW = 5


class SortPoolModel(object):
    def __init__(self, num_features, num_classes, seed=0, k=K, fused=False):
        dev = torch.device("cuda")
        self.k, self.fused = k, fused
        self.gcns = [tfg.layers.GCN(UNITS, activation=tfg.relu, seed=seed + level) for level in range(3)]
        for level, gcn in enumerate(self.gcns):
            gcn._maybe_build([torch.empty(1, num_features if level == 0 else UNITS)])
            gcn.trainable(True)
        self.sort_pool = tfg.layers.SortPool(k=k)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        steps = k - WINDOW + 1
        self.conv = (_glorot(gen, WINDOW * UNITS, UNITS, dev), torch.zeros(UNITS, device=dev, requires_grad=True))
        self.mlp = [(_glorot(gen, steps * UNITS, 128, dev), torch.zeros(128, device=dev, requires_grad=True)),
                    (_glorot(gen, 128, num_classes, dev), torch.zeros(num_classes, device=dev, requires_grad=True))]

    def parameters(self):
        ps = []
        for layer in self.gcns:
            ps += layer.parameters()
        for k, b in [self.conv] + self.mlp:
            ps += [k, b]
        return ps

    def head(self, h3, training):
        """[G, k, 128] -> logits: Conv1D(128, 5, relu, valid) as a window view and one dense product, Flatten, the MLP."""
        G, k, F = h3.shape
        steps = k - WINDOW + 1
        windows = torch.cat([h3[:, j:j + steps, :] for j in range(WINDOW)], dim=-1)           # [G, steps, WINDOW * F]
        kc, bc = self.conv
        h = AG.linear(windows.reshape(G * steps, WINDOW * F), kc, bc, tfg._lib.ACT_RELU).reshape(G, steps * UNITS)
        (k0, b0), (k1, b1) = self.mlp
        h = AG.linear(h, k0, b0, tfg._lib.ACT_RELU)
        if training:
            h = torch.nn.functional.dropout(h, 0.5, training=True)
        return AG.linear(h, k1, b1)

    def __call__(self, inputs, training=False):
        x, edge_index, node_graph_index, num_graphs = inputs
        h = x
        for gcn in self.gcns:
            h = gcn([h, edge_index, None], training=training)
        if self.fused:
            h3 = self.sort_pool.pool_3d([h, node_graph_index], num_graphs=num_graphs)
        else:
            pooled_x, _, _, pooled_node_graph_index = self.sort_pool([h, edge_index, None, node_graph_index], training=training)
            # the reference passes the UNPOOLED node_graph_index here (demo/demo_sort_pool.py:96), which only runs by accident
            # of shapes (a scatter index longer than its updates); the evident intent is the pooled rows' own graph index
            h3 = tfg.utils.convert_x_to_3d(pooled_x, pooled_node_graph_index, k=self.k, num_sources=num_graphs)
        return self.head(h3, training)


def static_logits(model, batch, training=False):
    """The model on a StaticBatchGraph: one row of logits per SLOT (a dead slot's [k, F] block is exactly zero)."""
    h = batch.x
    for gcn in model.gcns:
        h = gcn([h, batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
    return model.head(model.sort_pool.pool_static(h, batch), training)


def static_loss(model, batch, training=True):
    """Mean cross-entropy over the LIVE slots (a dead slot holds graph 0's label: torch.where on graph_mask)."""
    per_slot = torch.nn.functional.cross_entropy(static_logits(model, batch, training=training), batch.y.reshape(-1),
                                                 reduction="none")
    zero = torch.zeros((), dtype=per_slot.dtype, device=per_slot.device)
    return torch.where(batch.graph_mask, per_slot, zero).sum() / batch.counts[0].clamp(min=1).to(per_slot.dtype)


def evaluate(model, batches):
    correct = total = 0
    with torch.no_grad():
        for x, ei, gid, y, num_graphs in batches:
            pred = model([x, ei, gid, num_graphs]).argmax(-1)
            correct += int((pred == y).sum().item())
            total += int(y.shape[0])
    return correct / max(total, 1)


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
    loss = torch.nn.functional.cross_entropy(model([x, ei, gid, num_graphs], training=True), y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.item())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--fused", action="store_true", help="SortPool.pool_3d instead of SortPool + convert_x_to_3d")
    p.add_argument("--static", action="store_true", help="fixed-shape batches: collate_static and SortPool.pool_static")
    p.add_argument("--capture", action="store_true", help="replay the whole step from one hipGraph (implies --static)")
    args = p.parse_args()
    torch.manual_seed(args.seed)
    data = make_dataset(args.graphs, args.seed)
    n_test = len(data.graphs) // 10
    train_idx = np.arange(n_test, len(data.graphs))
    test_batches = [make_batch(data, list(range(i, min(i + args.batch_size, n_test)))) for i in range(0, n_test, args.batch_size)]
    model = SortPoolModel(data.num_features, data.num_classes, seed=args.seed, fused=args.fused or args.static or args.capture)
    if args.static or args.capture:
        return train_static(model, data, train_idx, test_batches, args)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    print("readout: {}".format("SortPool.pool_3d" if args.fused else "SortPool, then convert_x_to_3d"), flush=True)
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
