# coding=utf-8
"""Graph auto-encoder for link prediction (https://arxiv.org/abs/1611.07308) — the counterpart of the reference's
demo/demo_gae.py on a synthetic planted-partition graph.

    split     tfg.utils.edge_train_test_split: upper-triangular unique edges, seeded permutation on the device
    encoder   2-layer GCN over the TRAIN edges (both directions); its plan is built once
    decoder   tfg.nn.edge_dot: logit[e] = <z[row[e]], z[col[e]]>, one launch per list, no [E, F] intermediates
    negatives tfg.utils.negative_sampling: fresh pairs every step from the device-side rejection sampler (the sorted
              adjacency of the full graph is built once and memoised on the edge_index tensor)

Prints the loss per step and a rank-based AUC of held-out edges against fresh negatives.

    python examples/demo_gae.py [--nodes 20000] [--steps 60]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd.synthetic import planted_partition_graph   # noqa: E402


def rank_auc(pos_score, neg_score):
    """P(score of a positive > score of a negative) from ranks (Mann-Whitney U; ties broken by position)."""
    scores = torch.cat([pos_score, neg_score])
    ranks = torch.empty_like(scores)
    ranks[torch.argsort(scores)] = torch.arange(1, scores.numel() + 1, dtype=scores.dtype, device=scores.device)
    p, q = pos_score.numel(), neg_score.numel()
    return float((ranks[:p].sum() - p * (p + 1) / 2.0) / (p * q))


def main(nodes=20000, steps=60, seed=0, test_size=0.15, verbose=True):
    torch.manual_seed(seed)
    x_np, ei_np, _ = planted_partition_graph(nodes, seed=seed)
    x = tfg._lib.as_f32(x_np)
    edge_index = tfg._lib.as_i32(ei_np)                       # the full graph: what negatives must avoid
    train_ei, test_ei, _, _ = tfg.utils.edge_train_test_split(edge_index, test_size, seed=seed)
    graph_ei = torch.cat([train_ei, train_ei.flip(0)], dim=1).contiguous()      # message passing sees the train edges only
    graph_w = torch.ones(graph_ei.shape[1], device=x.device)
    cache = {}
    gcn0, gcn1 = tfg.layers.GCN(32, activation=tfg.relu), tfg.layers.GCN(16)

    def encode(training):
        h = gcn0([x, graph_ei, graph_w], cache=cache, training=training)
        return gcn1([h, graph_ei, graph_w], cache=cache, training=training)

    encode(False)                                             # builds the weights
    gcn0.trainable(True)
    gcn1.trainable(True)
    optimizer = torch.optim.Adam(gcn0.parameters() + gcn1.parameters(), lr=1e-2)
    num_pos = int(train_ei.shape[1])
    losses = []
    for step in range(1, steps + 1):
        optimizer.zero_grad()
        z = encode(True)
        neg_ei = tfg.utils.negative_sampling(num_pos, nodes, edge_index, seed=seed * 1000003 + step)
        pos_logit = tfg.nn.edge_dot(z, train_ei)              # its plan (for the backward) is memoised on train_ei
        neg_logit = tfg.nn.edge_dot(z, neg_ei)
        logits = torch.cat([pos_logit, neg_logit])
        labels = torch.cat([torch.ones_like(pos_logit), torch.zeros_like(neg_logit)])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        if verbose:
            print("step {} loss {:.4f}".format(step, losses[-1]))
    with torch.no_grad():
        z = encode(False)
        test_neg = tfg.utils.negative_sampling(int(test_ei.shape[1]), nodes, edge_index, seed=seed * 1000003 - 1)
        auc = rank_auc(tfg.nn.edge_dot(z, test_ei), tfg.nn.edge_dot(z, test_neg))
    print("test AUC {:.4f}".format(auc))
    return losses, auc


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    main(args.nodes, args.steps, args.seed)
