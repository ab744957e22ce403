# coding=utf-8
"""Mean-pool graph classification — the MI355X counterpart of the reference's demo/demo_mean_pool.py.

Same model: GCN(64, relu) -> Dropout(0.4) -> GCN(32, relu) -> mean readout -> Dropout(0.4) -> Dense(num_classes); Adam(lr 5e-3),
batches of 256 graphs.  NCI1 needs a download, so the data is the seeded NCI1-shaped stand-in of demo_sag_pool_h.py.

    python examples/demo_mean_pool.py [--steps 2000] [--static] [--capture]

The default route draws its batches from GraphStore.batches (one collate launch each; the step is issued launch by launch).
--static draws fixed-shape batches instead: a StaticLoader hands on graph ids from a device cursor, GraphStore.collate_static
assembles them at capacities the host computed once, and the readout takes the graph plan the batch carries — no host read
anywhere in the step.  --capture (implies --static) records ids -> batch -> forward -> loss -> backward -> Adam once with
tfg.CapturedTrainStep and replays it: every replay trains on the next batch.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd import autograd as AG   # noqa: E402
from demo_sag_pool_h import _glorot, make_dataset   # noqa: E402
from demo_graph_store import to_graphs   # noqa: E402

DROP_RATE = 0.4
NUM_GRAPHS, BATCH_SIZE, LEARNING_RATE, SEED = 4000, 256, 5e-3, 0


class MeanPoolNetwork(object):
    def __init__(self, num_features, num_classes, seed=0, drop_rate=DROP_RATE):
        dev = torch.device("cuda")
        self.drop_rate = float(drop_rate)
        self.gcn0 = tfg.layers.GCN(64, activation=tfg.relu, seed=seed)
        self.gcn1 = tfg.layers.GCN(32, activation=tfg.relu, seed=seed + 1)
        self.gcn0._maybe_build([torch.empty(1, num_features)])
        self.gcn1._maybe_build([torch.empty(1, 64)])
        for layer in (self.gcn0, self.gcn1):
            layer.trainable(True)
        gen = torch.Generator(device="cpu").manual_seed(seed + 100)
        self.dense = (_glorot(gen, 32, num_classes, dev), torch.zeros(num_classes, device=dev, requires_grad=True))

    def parameters(self):
        return self.gcn0.parameters() + self.gcn1.parameters() + list(self.dense)

    def __call__(self, batch, training=False):
        """Logits, one row per graph of a BatchGraph and one per SLOT of a StaticBatchGraph (dead slots: the bias alone)."""
        dropping = training and self.drop_rate > 0.0
        drop = (lambda h: torch.nn.functional.dropout(h, self.drop_rate, training=True)) if dropping else (lambda h: h)
        h = self.gcn0([batch.x, batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
        h = self.gcn1([drop(h), batch.edge_index, batch.edge_weight], cache=batch.cache, training=training)
        if isinstance(batch, tfg.data.StaticBatchGraph):
            h = batch.readout(h, "mean")
        else:
            h = tfg.nn.mean_pool(h, batch.node_graph_index, batch.num_graphs, cache=batch.cache)
        return AG.linear(drop(h), *self.dense)


def batch_loss(model, batch, training=True):
    """Mean cross-entropy over the graphs of the batch; on a static batch over its live slots (torch.where on graph_mask: a
    dead slot holds graph 0's label and must not count)."""
    logits = model(batch, training=training)
    y = batch.y.reshape(-1)
    if not isinstance(batch, tfg.data.StaticBatchGraph):
        return torch.nn.functional.cross_entropy(logits, y)
    per_slot = torch.nn.functional.cross_entropy(logits, y, reduction="none")
    zero = torch.zeros((), dtype=per_slot.dtype, device=per_slot.device)
    return torch.where(batch.graph_mask, per_slot, zero).sum() / batch.counts[0].clamp(min=1).to(per_slot.dtype)


def make_static_loss_fn(model, store, loader, capacities):
    """The whole data side of a step as device work: next ids -> collate_static -> loss.  What CapturedTrainStep records."""
    def loss_fn():
        return batch_loss(model, store.collate_static(loader.next_ids(), capacities))
    return loss_fn


def evaluate(model, store, batch_size):
    correct = total = 0
    with torch.no_grad():
        for b in store.batches(batch_size):
            correct += int((model(b).argmax(-1) == b.y.reshape(-1)).sum().item())
            total += b.num_graphs
    return correct / max(total, 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--static", action="store_true", help="fixed-shape batches (collate_static over a device-side loader)")
    p.add_argument("--capture", action="store_true", help="replay the whole step from one hipGraph (implies --static)")
    args = p.parse_args()
    static = args.static or args.capture
    torch.manual_seed(SEED)
    data = make_dataset(NUM_GRAPHS, SEED)
    n_test = len(data.graphs) // 10
    train_store = tfg.data.GraphStore(to_graphs(data, range(n_test, len(data.graphs))))
    test_store = tfg.data.GraphStore(to_graphs(data, range(n_test)))
    model = MeanPoolNetwork(data.num_features, data.num_classes, seed=SEED)
    opt = torch.optim.Adam(model.parameters(), lr=LEARNING_RATE, capturable=args.capture)
    print("batches: {}".format("collate_static, replayed" if args.capture else "collate_static" if static
                               else "GraphStore.batches"), flush=True)

    if static:
        loader = train_store.static_loader(BATCH_SIZE, shuffle=True, seed=SEED + 1)
        cap = train_store.static_capacities(BATCH_SIZE)
        loss_fn = make_static_loss_fn(model, train_store, loader, cap)
        if args.capture:
            step = tfg.CapturedTrainStep(loss_fn, opt)
            loader.cursor.zero_()                 # the warm-up steps advanced it
        else:
            def step():
                opt.zero_grad(set_to_none=True)
                loss = loss_fn()
                loss.backward()
                opt.step()
                return loss
        print("capacities: {} rows and {} edges for {} slots".format(cap.n_cap, cap.e_cap, cap.batch_size), flush=True)
    else:
        def batches():
            epoch = 0
            while True:
                for b in train_store.batches(BATCH_SIZE, shuffle=True, seed=SEED + 1 + epoch):
                    yield b
                epoch += 1
        stream = batches()

        def step():
            opt.zero_grad(set_to_none=True)
            loss = batch_loss(model, next(stream))
            loss.backward()
            opt.step()
            return loss

    report = max(1, min(20, args.steps // 3))
    window, t0 = [], time.perf_counter()
    for i in range(args.steps):
        if static and i and i % loader.steps_per_epoch == 0:
            loader.reshuffle(SEED + 1 + i // loader.steps_per_epoch)       # in place: the replay reads the new order
        window.append(step().detach().clone())
        if (i + 1) % report == 0 or i + 1 == args.steps:
            loss = float(torch.stack(window).mean().item())                       # the one read of the window
            ms = (time.perf_counter() - t0) * 1e3 / len(window)
            print("step {:5d}  loss {:.4f}  accuracy {:.4f}  ({:.2f} ms / step)".format(
                i + 1, loss, evaluate(model, test_store, BATCH_SIZE), ms), flush=True)
            window, t0 = [], time.perf_counter()


if __name__ == "__main__":
    main()
