# coding=utf-8
"""LSTM GraphSAGE aggregator: forward and forward + backward time of nn.lstm_graph_sage beside its two roofs.

    python tools/bench_lstm_sage.py [--shape batch|products|both] [--units 64] [--features 100] [--k 25] [--rounds 5]
                                    [--out profiles/lstm_sage.jsonl]

Shapes: `batch` = a sampled mini-batch (--batch-nodes destinations, k sampled neighbours each, over --nodes sources);
`products` = every node of an ogbn-products-sized graph (N = 2 449 029) with k = 25 sampled neighbours (forward only: the
training state is 20 U bytes per (row, step)).  Roofs: `mfma_ms` = the recurrent product's N T 8 U^2 FLOPs at the f32-MFMA
peak (--mfma-tflops, 157.3); `gather_ms` = the N T gathered P rows of 16 U bytes at --hbm-tbs (8.0).  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(n_dst, n_src, k, F, U, rounds, backward, args):
    dev = tfg._lib.device()
    g = torch.Generator().manual_seed(1)
    row = torch.arange(n_dst, dtype=torch.int32).repeat_interleave(k)
    col = torch.randint(0, n_src, (n_dst * k,), generator=g, dtype=torch.int32)
    ei = torch.stack([row, col]).to(dev)
    x = torch.randn(n_src, F, generator=g).to(dev)
    layer = tfg.layers.LSTMGraphSage(2 * U, seed=1)
    cache = {}
    layer([x, ei], cache=cache)
    fwd = [event_ms(lambda: layer([x, ei], cache=cache)) for _ in range(rounds + 1)][1:]
    out = dict(n_dst=n_dst, n_src=n_src, T=k, F=F, U=U, forward_ms=round(float(np.median(fwd)), 4),
               mfma_ms=round(n_dst * k * 8.0 * U * U / (args.mfma_tflops * 1e9), 4),
               gather_ms=round(n_dst * k * 16.0 * U / (args.hbm_tbs * 1e9), 4))
    if backward:
        layer.trainable(True)

        def step():
            for p in layer.parameters():
                p.grad = None
            layer([x, ei], cache=cache).sum().backward()
        both = [event_ms(step) for _ in range(rounds + 1)][1:]
        out["forward_backward_ms"] = round(float(np.median(both)), 4)
        out["saved_bytes"] = int(tfg._lib.load_library().tfgx_lstm_aggregate_saved_bytes(n_dst, k, U))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["batch", "products", "both"])
    ap.add_argument("--units", type=int, default=64)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--nodes", type=int, default=2449029)
    ap.add_argument("--batch-nodes", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-tflops", type=float, default=157.3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(tool="bench_lstm_sage", device=torch.cuda.get_device_name(0))
    if args.shape in ("batch", "both"):
        n = args.batch_nodes
        res["batch"] = measure(n, n, args.k, args.features, args.units, args.rounds, True, args)
    if args.shape in ("products", "both"):
        res["products"] = measure(args.nodes, args.nodes, args.k, args.features, args.units, args.rounds, False, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
