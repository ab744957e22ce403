# coding=utf-8
"""2-layer MeanGraphSage trained on MINIBATCHES of seed nodes: per step, RandomNeighborSampler.sample_blocks draws the seeds'
sampled 2-hop neighbourhood (fan-outs 25, 10 as num_sampled_neighbors_list of the reference's demo/demo_graph_sage.py) and hands
each layer a small relabelled block with its CSR plan attached — the work of a step is proportional to the batch, not to the
graph (include/tfgx_nbrblock.h).  The graph is a planted-partition graph (tf_geometric_amd.synthetic): node classification.

--fuse-input-hop leaves the outermost hop to the fused sample-and-reduce kernel (include/tfgx_samplereduce.h): it is drawn and
reduced straight out of the feature table, and layer 0 finishes on the destination rows only (MeanGraphSage.combine).

--static samples with FIXED shapes (RandomNeighborSampler.sample_blocks_static, include/tfgx_nbrstatic.h): every step's tensors
have the capacity (batch, fan-outs) give, the short last batch of an epoch fills its seed list with -1 (dead slots) and the loss
is masked with mb.seed_mask; nothing is read back from the device.  --capture replays that whole step — sample, forward,
backward, Adam — from one hipGraph (tfg.CapturedTrainStep); the sampling seed is a device word the captured step advances.

--half-features bf16 | fp16 keeps the feature table in 16 bits (tfg.prepare_half_features(..., minibatch=True), on its line-friendly
row stride) and drops the float32 copy: the gather and the fused input hop read it in place (include/tfgx_minibatch_h16.h) and
return float32 rows, bit for bit what they return for the table widened to float32.  It composes with every flag above.

    python examples/demo_graph_sage_minibatch.py [--epochs 5] [--batch 256] [--fuse-input-hop] [--static | --capture]
                                                 [--half-features bf16|fp16]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd.synthetic import planted_partition_graph   # noqa: E402
from tf_geometric_amd.utils import RandomNeighborSampler   # noqa: E402

FANOUTS = [25, 10]               # fanouts[l] belongs to layer l, input side first
HALF_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def main(epochs=5, batch=256, num_nodes=20000, classes=6, quiet=False, fuse_input_hop=False, static=False, capture=False,
         half_features=None):
    static = static or capture
    torch.manual_seed(0)
    x_np, ei_np, y_np = planted_partition_graph(num_nodes, classes=classes, degree=12, features=32, seed=0)
    # extra feature noise: a node's own row says little about its class, the mean over its (mostly same-class) neighbours does
    x_np = x_np + 3.0 * np.random.Generator(np.random.PCG64(1)).standard_normal(x_np.shape).astype(np.float32)
    x, y = tfg._lib.as_f32(x_np), torch.from_numpy(y_np).to(tfg._lib.device())
    if half_features is not None:                                    # the table every step gathers from, in 16 bits from here on
        x = tfg.prepare_half_features(x, HALF_DTYPES[half_features], minibatch=True)
    sampler = RandomNeighborSampler(tfg._lib.as_i32(ei_np))          # device tensors in -> device tensors out
    perm = torch.randperm(num_nodes)
    train_ids, test_ids = perm[:num_nodes * 4 // 5], perm[num_nodes * 4 // 5:]
    layers = [tfg.layers.MeanGraphSage(units=64, activation=tfg.relu, concat=True).trainable(True),
              tfg.layers.MeanGraphSage(units=64, activation=tfg.relu, concat=True).trainable(True)]
    fc = torch.nn.Linear(64, classes).cuda()

    def forward_fused(seeds, training):
        mb = sampler.sample_blocks(seeds, FANOUTS, fuse_input_hop=True)      # the hops but the outermost; one host read fewer
        h = layers[0].combine([mb.gather(x), mb.input_aggregate(x, "mean")], training=training)
        for layer, b in zip(layers[1:], mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=training)[:b.num_dst]
        return fc(h)

    def forward(seeds, training):
        if fuse_input_hop:
            return forward_fused(seeds, training)
        mb = sampler.sample_blocks(seeds, FANOUTS)                  # a fresh sample per step (seed from torch's generator)
        h = mb.gather(x)
        for layer, b in zip(layers, mb.blocks):
            # the layer sees the block's num_src nodes; only its first num_dst rows have their neighbourhood
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=training)[:b.num_dst]
        return fc(h)

    # the fixed-shape route: the step reads its batch from buffers that keep their addresses and its sampling seed from a
    # device word it advances itself, so the same launch sequence serves every step (and a hipGraph can replay it)
    seeds_buf = torch.full((batch,), -1, dtype=torch.int32, device=y.device)
    labels_buf = torch.zeros(batch, dtype=y.dtype, device=y.device)
    seed_state = torch.full((1,), 20240, dtype=torch.int64, device=y.device)

    def load_batch(seeds):
        n = int(seeds.shape[0])                                     # the short last batch: the rest are dead slots
        seeds_buf.fill_(-1)
        seeds_buf[:n] = seeds.to(seeds_buf.device, torch.int32)
        labels_buf.zero_()
        labels_buf[:n] = y[seeds.to(y.device)]

    def static_loss():
        mb = sampler.sample_blocks_static(seeds_buf, FANOUTS, seed=seed_state, fuse_input_hop=fuse_input_hop)
        seed_state.add_(1)
        h, rest = mb.gather(x), layers
        if fuse_input_hop:
            h, rest = layers[0].combine([h, mb.input_aggregate(x, "mean")], training=True), layers[1:]
        for layer, b in zip(rest, mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        per_seed = torch.nn.functional.cross_entropy(fc(h[:batch]), labels_buf, reduction="none")
        return (per_seed * mb.seed_mask).sum() / mb.seed_mask.sum().clamp(min=1)       # dead slots carry no loss

    with torch.no_grad():
        forward(train_ids[:8], False)                               # lazy weight build
    opt = torch.optim.Adam([p for s in layers for p in s.parameters()] + list(fc.parameters()), lr=1e-2, capturable=capture)
    captured = None
    if capture:
        load_batch(train_ids[:batch])                               # the warm-up steps of the capture run on a real batch
        captured = tfg.CapturedTrainStep(static_loss, opt)          # (they are rolled back; the sampler's state now exists)
    acc, loss = 0.0, None
    for epoch in range(epochs):
        order = train_ids[torch.randperm(train_ids.shape[0])]
        for i in range(0, order.shape[0], batch):
            seeds = order[i:i + batch]
            if capture:
                load_batch(seeds)
                loss = captured()                                   # a device scalar: nothing is read until it is printed
                continue
            opt.zero_grad()
            if static:
                load_batch(seeds)
                loss = static_loss()
            else:
                loss = torch.nn.functional.cross_entropy(forward(seeds, True), y[seeds.to(y.device)])
            loss.backward()
            opt.step()
        with torch.no_grad():
            hits = sum(int((forward(test_ids[i:i + 1024], False).argmax(1) == y[test_ids[i:i + 1024].to(y.device)]).sum())
                       for i in range(0, test_ids.shape[0], 1024))
            acc = hits / float(test_ids.shape[0])
        if not quiet:
            print("epoch = {}\tloss = {:.4f}\ttest_accuracy = {:.4f}".format(epoch, float(loss.detach()), acc))
    return acc, float(loss.detach())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--fuse-input-hop", action="store_true", help="draw and reduce the outermost hop in one launch")
    ap.add_argument("--static", action="store_true", help="fixed-shape sampling: no host read, dead slots, a masked loss")
    ap.add_argument("--capture", action="store_true", help="--static, the whole step replayed from one hipGraph")
    ap.add_argument("--half-features", choices=sorted(HALF_DTYPES), default=None,
                    help="keep the feature table in 16 bits; the gather and the fused input hop read it in place")
    args = ap.parse_args()
    main(epochs=args.epochs, batch=args.batch, fuse_input_hop=args.fuse_input_hop, static=args.static or args.capture,
         capture=args.capture, half_features=args.half_features)
