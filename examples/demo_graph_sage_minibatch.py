# coding=utf-8
"""2-layer MeanGraphSage trained on MINIBATCHES of seed nodes: per step, RandomNeighborSampler.sample_blocks draws the seeds'
sampled 2-hop neighbourhood (fan-outs 25, 10 as num_sampled_neighbors_list of the reference's demo/demo_graph_sage.py) and hands
each layer a small relabelled block with its CSR plan attached — the work of a step is proportional to the batch, not to the
graph (include/tfgx_nbrblock.h).  The graph is a planted-partition graph (tf_geometric_amd.synthetic): node classification.

--fuse-input-hop leaves the outermost hop to the fused sample-and-reduce kernel (include/tfgx_samplereduce.h): it is drawn and
reduced straight out of the feature table, and layer 0 finishes on the destination rows only (MeanGraphSage.combine).

    python examples/demo_graph_sage_minibatch.py [--epochs 5] [--batch 256] [--fuse-input-hop]
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


def main(epochs=5, batch=256, num_nodes=20000, classes=6, quiet=False, fuse_input_hop=False):
    torch.manual_seed(0)
    x_np, ei_np, y_np = planted_partition_graph(num_nodes, classes=classes, degree=12, features=32, seed=0)
    # extra feature noise: a node's own row says little about its class, the mean over its (mostly same-class) neighbours does
    x_np = x_np + 3.0 * np.random.Generator(np.random.PCG64(1)).standard_normal(x_np.shape).astype(np.float32)
    x, y = tfg._lib.as_f32(x_np), torch.from_numpy(y_np).to(tfg._lib.device())
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

    with torch.no_grad():
        forward(train_ids[:8], False)                               # lazy weight build
    opt = torch.optim.Adam([p for s in layers for p in s.parameters()] + list(fc.parameters()), lr=1e-2)
    acc, loss = 0.0, None
    for epoch in range(epochs):
        order = train_ids[torch.randperm(train_ids.shape[0])]
        for i in range(0, order.shape[0], batch):
            seeds = order[i:i + batch]
            opt.zero_grad()
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
    args = ap.parse_args()
    main(epochs=args.epochs, batch=args.batch, fuse_input_hop=args.fuse_input_hop)
