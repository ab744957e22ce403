# coding=utf-8
"""Set2Set's attention readout: the fused launch (tfgx_set2set_attend_f32 and its backward) beside the same values composed
from the operators the package had before it — tfg.nn.segment_softmax, tfg.nn.sum_pool and torch elementwise ops, the
decomposition of the reference's nn/pool/set2set.py:35-39 — and the whole nn.set2set call in both modes.

    python tools/bench_set2set.py [--nodes 1000000] [--features 64] [--graph-nodes 30] [--rounds 10] [--out FILE]

Each configuration is timed forward and forward + backward, A and B alternating, with sorted and with shuffled graph ids,
for TU-sized graphs (--graph-nodes nodes each) and for ONE graph of all the nodes.  `floor_ms` is the readout's
compulsory traffic (4 N F bytes forward, 8 N F more backward) at --hbm-tbs.  A measurement tool: it has no pass / fail
ratio.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd import autograd as AG   # noqa: E402
from tf_geometric_amd.nn.pool.set2set import _graph_plan   # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def composed(x, ids, q, G):
    """set2set.py:35-39 on the operators that exist without the fused kernel."""
    repeated = q[ids.long()]
    score = (x * repeated).sum(-1, keepdim=True)
    normed = tfg.nn.segment_softmax(score, ids, G)
    return tfg.nn.sum_pool(x * normed, ids, G)


def alternate(fa, fb, rounds):
    fa(), fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    return round(float(np.median(ta)), 4), round(float(np.median(tb)), 4)


def readout(N, F, G, shuffled, rounds, hbm_tbs):
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(1)
    ids = (torch.arange(N) * G // N).to(torch.int32)
    if shuffled:
        ids = ids[torch.randperm(N, generator=g)]
    ids = ids.to(dev)
    x = torch.randn(N, F, generator=g).to(dev)
    q = torch.randn(G, F, generator=g).to(dev)
    plan = _graph_plan(ids, G, N, None)
    with torch.no_grad():
        fused_ms, composed_ms = alternate(lambda: AG.set2set_attend(plan, x, q), lambda: composed(x, ids, q, G), rounds)
        err = float((AG.set2set_attend(plan, x, q) - composed(x, ids, q, G)).abs().max())
    xg, qg = x.clone().requires_grad_(True), q.clone().requires_grad_(True)

    def train(fn):
        xg.grad = qg.grad = None
        fn().sum().backward()
    fused_fb, composed_fb = alternate(lambda: train(lambda: AG.set2set_attend(plan, xg, qg)),
                                      lambda: train(lambda: composed(xg, ids, qg, G)), rounds)
    return dict(N=N, F=F, G=G, shuffled=shuffled, fused_forward_ms=fused_ms, composed_forward_ms=composed_ms,
                fused_forward_backward_ms=fused_fb, composed_forward_backward_ms=composed_fb, max_abs_difference=err,
                floor_forward_ms=round(4.0 * N * F / (hbm_tbs * 1e9), 4), floor_forward_backward_ms=round(12.0 * N * F / (hbm_tbs * 1e9), 4))


def whole(N, F, G, batch_graphs, iterations, rounds):
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(2)
    ids = (torch.arange(N) * G // N).to(torch.int32).to(dev)
    x = torch.randn(N, F, generator=g).to(dev)
    layer = tfg.layers.Set2Set(num_iterations=iterations, batch_graphs=batch_graphs, seed=1)
    cache = {}
    layer([x, ids, G], cache=cache)
    with torch.no_grad():
        fwd = [event_ms(lambda: layer([x, ids, G], cache=cache)) for _ in range(rounds + 1)][1:]
    layer.trainable(True)

    def step():
        for p in layer.parameters():
            p.grad = None
        layer([x, ids, G], cache=cache).sum().backward()
    both = [event_ms(step) for _ in range(rounds + 1)][1:]
    return dict(N=N, F=F, G=G, batch_graphs=batch_graphs, num_iterations=iterations, forward_ms=round(float(np.median(fwd)), 4),
                forward_backward_ms=round(float(np.median(both)), 4),
                lstm_steps_per_launch=1 if batch_graphs else G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--graph-nodes", type=int, default=30)
    ap.add_argument("--set2set-graphs", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, F = args.nodes, args.features
    res = dict(tool="bench_set2set", device=torch.cuda.get_device_name(0), readout=[], set2set=[])
    for G in (max(N // args.graph_nodes, 1), 1):
        for shuffled in (False, True):
            res["readout"].append(readout(N, F, G, shuffled, args.rounds, args.hbm_tbs))
    G = args.set2set_graphs
    for batch_graphs in (False, True):
        res["set2set"].append(whole(G * args.graph_nodes, F, G, batch_graphs, args.iterations, args.rounds))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
