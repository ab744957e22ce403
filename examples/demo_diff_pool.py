# coding=utf-8
"""Hierarchical DiffPool graph classification — the MI355X counterpart of the reference's demo/demo_diff_pool.py.

Same model: two DiffPool levels with 20 and 5 clusters per graph; at each level a feature GNN (two GCN(128, relu)) and an
assignment GNN (GCN(128, relu) -> GCN(num_clusters)), a mean || max readout of the pooled graph after every level, the
readouts concatenated, Dropout(0.5) -> Dense(num_classes); Adam(lr 1e-3), batches of 50 graphs.  NCI1 needs a download, so
the data is the seeded NCI1-shaped stand-in of examples/demo_sag_pool_h.py.

    python examples/demo_diff_pool.py [--steps 40] [--graphs 600] [--static] [--capture]

Every S^T A S, S^T h product runs on the segmented-product kernel (include/tfgx_seggram.h); each pooled edge list carries its
CSR plan, so the second level does not sort.  As in the reference, the pooled edge weights are differentiable in the
assignment and train through the second level's GCNs: the GCN normalisation differentiates an edge_weight that requires
grad (include/tfgx_normgrad.h).

--static trains on fixed-shape batches instead: a GraphStore holds the graphs on the device, a StaticLoader hands on graph ids
from a device cursor, collate_static assembles them at capacities the host computed once, and every level is the layer's
pool_static (a static batch in, a static batch of B K rows and B K K edges out: include/tfgx_dense_pool_static.h) with the
readouts the batches carry and a loss masked by graph_mask — no host read anywhere in the step.  --capture (implies --static)
records ids -> batch -> both levels -> loss -> backward -> Adam once with tfg.CapturedTrainStep and replays it.  Without either
flag the program is what it was.
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
from demo_sag_pool_h import make_dataset, make_batch, _glorot, graph_store, make_static_step   # noqa: E402

NUM_CLUSTERS = [20, 5]
UNITS = 128


class GcnStack(object):
    """[x, edge_index, edge_weight] -> h through GCN layers; the call shape the pooling layers expect of a GNN."""

    def __init__(self, num_features, units_list, last_activation, seed):
        self.gcns = []
        for i, units in enumerate(units_list):
            act = tfg.relu if (i < len(units_list) - 1 or last_activation) else None
            gcn = tfg.layers.GCN(units, activation=act, seed=seed + i)
            gcn._maybe_build([torch.empty(1, num_features if i == 0 else units_list[i - 1])])
            gcn.trainable(True)
            self.gcns.append(gcn)

    def parameters(self):
        return [p for gcn in self.gcns for p in gcn.parameters()]

    def __call__(self, inputs, training=None, cache=None):
        h, edge_index, edge_weight = inputs
        for gcn in self.gcns:
            h = gcn([h, edge_index, edge_weight], training=training)
        return h


class CachedGcnStack(GcnStack):
    """The same stack handing the `cache` it is given to every GCN: pool_static passes the static batch's, which carries the
    batch's plans (and, for weights that are not being trained, the normalised adjacency of the first GCN for the others)."""

    def __call__(self, inputs, training=None, cache=None):
        h, edge_index, edge_weight = inputs
        for gcn in self.gcns:
            h = gcn([h, edge_index, edge_weight], training=training, cache=cache)
        return h


class DensePoolModel(object):
    """detach_pooled_weights: hand the pooled edge weights to the next level as constants — for a pooling layer that refuses
    an edge_weight that requires grad (MinCutPool); DiffPool trains through them."""

    def __init__(self, pool_cls, num_features, num_classes, seed=0, detach_pooled_weights=False, stack=GcnStack):
        dev = torch.device("cuda")
        self.detach_pooled_weights = detach_pooled_weights
        self.gnns, self.pools = [], []
        for level, k in enumerate(NUM_CLUSTERS):
            f = num_features if level == 0 else UNITS
            feature = stack(f, [UNITS, UNITS], True, seed + 10 * level)
            assign = stack(f, [UNITS, k], False, seed + 10 * level + 5)
            pool = pool_cls(feature, assign, UNITS, k, activation=torch.relu)
            pool.trainable(True)
            self.gnns += [feature, assign]
            self.pools.append(pool)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.head = (_glorot(gen, 2 * UNITS * len(NUM_CLUSTERS), num_classes, dev),
                     torch.zeros(num_classes, device=dev, requires_grad=True))

    def parameters(self):
        return [p for m in self.gnns + self.pools for p in m.parameters()] + list(self.head)

    def __call__(self, inputs, training=False, return_losses=False):
        h, edge_index, node_graph_index, num_graphs = inputs
        edge_weight, readouts, losses = None, [], []
        for pool in self.pools:
            out = pool([h, edge_index, edge_weight, node_graph_index], training=training, num_graphs=num_graphs,
                       **(dict(return_loss_func=True) if return_losses else {}))
            if return_losses:
                out, loss_func = out
                losses.append(loss_func())
            h, edge_index, edge_weight, node_graph_index = out
            if self.detach_pooled_weights:
                edge_weight = edge_weight.detach()
            readouts.append(torch.cat([tfg.nn.mean_pool(h, node_graph_index, num_graphs),
                                       tfg.nn.max_pool(h, node_graph_index, num_graphs)], dim=-1))
        g = torch.cat(readouts, dim=-1)
        if training:
            g = torch.nn.functional.dropout(g, 0.5, training=True)
        logits = AG.linear(g, *self.head)
        return (logits, losses) if return_losses else logits

    def static(self, batch, training=False, return_losses=False):
        """The model on a StaticBatchGraph: one row of logits per SLOT (dead slots: the biases alone).  Level by level the
        pooled batch replaces its parent; mean || max readouts through the graph plan each batch carries."""
        h, readouts, losses = batch.x, [], []
        for pool in self.pools:
            if return_losses:
                batch, pair = pool.pool_static(h, batch, training=training, return_losses=True)
                losses.append(pair)
            else:
                batch = pool.pool_static(h, batch, training=training)
            if self.detach_pooled_weights:
                batch.edge_weight = batch.edge_weight.detach()
            h = batch.x
            readouts.append(torch.cat([batch.readout(h, "mean"), batch.readout(h, "max")], dim=-1))
        g = torch.cat(readouts, dim=-1)
        if training:
            g = torch.nn.functional.dropout(g, 0.5, training=True)
        logits = AG.linear(g, *self.head)
        return (logits, losses) if return_losses else logits


def static_loss(with_losses):
    """loss(model, batch): the mean cross-entropy over the LIVE slots (a dead slot holds graph 0's label: torch.where on
    graph_mask) plus, with_losses, every level's cut and orthogonality loss (means over the live slots themselves)."""
    def loss(model, batch, training=True):
        out = model.static(batch, training=training, return_losses=with_losses)
        logits, losses = out if with_losses else (out, [])
        per_slot = torch.nn.functional.cross_entropy(logits, batch.y.reshape(-1), reduction="none")
        zero = torch.zeros((), dtype=per_slot.dtype, device=per_slot.device)
        total = torch.where(batch.graph_mask, per_slot, zero).sum() / batch.counts[0].clamp(min=1).to(per_slot.dtype)
        for cut, orth in losses:
            total = total + cut + orth
        return total
    return loss


def run_static(pool_cls, with_losses, detach_pooled_weights, data, args):
    """The --static / --capture route: the steps of run() over fixed-shape batches."""
    model = DensePoolModel(pool_cls, data.num_features, data.num_classes, seed=args.seed,
                           detach_pooled_weights=detach_pooled_weights, stack=CachedGcnStack)
    store = graph_store(data, range(len(data.graphs)))
    loader = store.static_loader(args.batch_size, shuffle=True, seed=args.seed + 1)
    cap = store.static_capacities(args.batch_size)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, capturable=args.capture)
    step = make_static_step(model, store, loader, cap, opt, args.capture, loss=static_loss(with_losses))
    print("batches: collate_static{}; capacities: {} rows and {} edges for {} slots, pooled to {} and {} rows".format(
        ", replayed" if args.capture else "", cap.n_cap, cap.e_cap, cap.batch_size,
        *[cap.batch_size * k for k in NUM_CLUSTERS]), flush=True)
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        if i and i % loader.steps_per_epoch == 0:
            loader.reshuffle(args.seed + 1 + i)                   # in place: the replay reads the new order
        loss = step()
        if i % 5 == 0 or i == args.steps - 1:
            value = float(loss.detach())                          # the one read, on the steps that print
            print("step {:4d}  loss {:.4f}  ({:.1f} ms / step)".format(i, value, (time.perf_counter() - t0) * 1e3 / (i + 1)),
                  flush=True)
    assert torch.isfinite(loss), "the loss diverged"


def run(pool_cls, with_losses, title, detach_pooled_weights=False):
    p = argparse.ArgumentParser(description=title)
    p.add_argument("--graphs", type=int, default=600)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--batch-size", type=int, default=50)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--static", action="store_true", help="fixed-shape batches: collate_static and the layers' pool_static")
    p.add_argument("--capture", action="store_true", help="replay the whole step from one hipGraph (implies --static)")
    args = p.parse_args()
    torch.manual_seed(args.seed)
    data = make_dataset(args.graphs, args.seed)
    if args.static or args.capture:
        return run_static(pool_cls, with_losses, detach_pooled_weights, data, args)
    model = DensePoolModel(pool_cls, data.num_features, data.num_classes, seed=args.seed,
                           detach_pooled_weights=detach_pooled_weights)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.Generator(np.random.PCG64(args.seed + 1))
    t0 = time.perf_counter()
    for step in range(args.steps):
        x, ei, gid, y, num_graphs = make_batch(data, list(rng.choice(len(data.graphs), args.batch_size, replace=False)))
        if with_losses:
            logits, losses = model([x, ei, gid, num_graphs], training=True, return_losses=True)
            cut_loss, orth_loss = sum(c for c, _ in losses), sum(o for _, o in losses)
        else:
            logits = model([x, ei, gid, num_graphs], training=True)
            cut_loss = orth_loss = torch.zeros((), device=logits.device)
        cls_loss = torch.nn.functional.cross_entropy(logits, y)
        loss = cls_loss + cut_loss + orth_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 5 == 0 or step == args.steps - 1:
            torch.cuda.synchronize()
            extra = "  cut_loss {:.4f}  orth_loss {:.4f}".format(float(cut_loss), float(orth_loss)) if with_losses else ""
            print("step {:4d}  loss {:.4f}{}  accuracy {:.3f}  ({:.1f} ms / step)".format(
                step, float(loss), extra, float((logits.argmax(-1) == y).float().mean()),
                (time.perf_counter() - t0) * 1e3 / (step + 1)), flush=True)
    assert torch.isfinite(loss), "the loss diverged"


if __name__ == "__main__":
    run(tfg.layers.DiffPool, False, "DiffPool on an NCI1-shaped synthetic set")
