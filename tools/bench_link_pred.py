# coding=utf-8
"""Link-prediction kernels: tfg.nn.edge_dot against the torch composition, and negative-sampler throughput.

    python tools/bench_link_pred.py [--nodes 2449029] [--edges 123718280] [--features 16,100,256] [--rounds 7]
                                    [--out profiles/link_pred_products.jsonl]

One process, variants interleaved round by round, device events around each variant, medians with the spread.  One JSON
line per measurement:
  edge_dot   ms of one tfgx_edge_dot_f32 launch over E uniform random pairs; algorithmic bytes E * (8 F + 12); the 128-byte
             lines the two gathers touch per second, and that rate as a fraction of --ceiling-glines (the random-line rate
             of DESIGN.md §2.1); `torch_ms` = (z[row] * z[col]).sum(-1) in torch, evaluated in edge chunks of --torch-chunk
             (its three [E, F] intermediates do not fit in memory at E = 123 M, F = 256) — the results are compared first
  sampler    ms and samples/s of negative_sampling (one launch + its host read) and negative_sampling_with_start_node on a
             graph of --nodes nodes and --sampler-edges edges; `dense_ms` = the reference's dense [N, N] construction
             (numpy, on the host) only where N * N * 8 bytes <= --dense-limit-bytes, else null"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), p25=round(float(np.percentile(v, 25)), 4),
                p75=round(float(np.percentile(v, 75)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_edge_dot(z, ei, chunk):
    out = torch.empty(ei.shape[1], dtype=torch.float32, device=z.device)
    for s in range(0, int(ei.shape[1]), chunk):
        r, c = ei[0, s:s + chunk].long(), ei[1, s:s + chunk].long()
        out[s:s + chunk] = (z[r] * z[c]).sum(-1)
    return out


def lines_per_row(F, ld):
    """Average number of 128-byte lines a row of F floats touches at row stride ld floats (rows start every 4 ld bytes)."""
    starts = (np.arange(32, dtype=np.int64) * ld * 4) % 128
    return float(np.mean((starts + F * 4 + 127) // 128))


def bench_edge_dot(n, e, F, rounds, chunk, ceiling, dev, emit):
    g = torch.Generator(device=dev)
    g.manual_seed(F)
    z = torch.randn((n, F), device=dev, generator=g)
    ei = torch.randint(0, n, (2, e), device=dev, generator=g, dtype=torch.int32)
    ours = tfg.nn.edge_dot(z, ei)                       # also reads the range flag once: later calls do not synchronise
    ref = torch_edge_dot(z, ei, chunk)
    worst = float((ours - ref).abs().max())
    t_ours, t_torch = [], []
    for _ in range(rounds):
        t_ours.append(event_ms(lambda: tfg.nn.edge_dot(z, ei))[0])
        t_torch.append(event_ms(lambda: torch_edge_dot(z, ei, chunk))[0])
    ms = float(np.median(t_ours))
    lines = 2.0 * e * lines_per_row(F, F)
    emit(dict(kind="edge_dot", nodes=n, edges=e, F=F, ms=stats(t_ours), torch_ms=stats(t_torch),
              speedup=round(float(np.median(t_torch)) / ms, 3), algorithmic_bytes=e * (8 * F + 12),
              algorithmic_gbps=round(e * (8 * F + 12) / ms / 1e6, 1), glines_per_s=round(lines / ms / 1e6, 2),
              fraction_of_ceiling=round(lines / ms / 1e6 / ceiling, 3), ceiling_glines=ceiling,
              max_abs_diff_vs_torch=worst))


def bench_sampler(n, graph_edges, samples, rounds, dense_limit, dev, emit):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    ei = torch.randint(0, n, (2, graph_edges), device=dev, generator=g, dtype=torch.int32)
    t0 = time.perf_counter()
    tfg.utils.sorted_adjacency(ei, n, undirected=True)
    tfg.utils.sorted_adjacency(ei, n, undirected=False)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    start = torch.randint(0, n, (samples,), device=dev, generator=g, dtype=torch.int32)
    t_pairs, t_from = [], []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tfg.utils.negative_sampling(samples, n, ei, seed=r)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tfg.utils.negative_sampling_with_start_node(start, n, ei, seed=r)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:                                           # round 0 warms up
            t_pairs.append((t1 - t0) * 1e3)
            t_from.append((t2 - t1) * 1e3)
    dense_ms = None
    if n * n * 8 <= dense_limit:                        # the reference's construction (graph_utils.py:391-400), on the host
        ei_np = ei.cpu().numpy()
        t0 = time.perf_counter()
        adj = np.triu(np.ones([n, n]), k=1)
        adj[np.minimum(ei_np[0], ei_np[1]), np.maximum(ei_np[0], ei_np[1])] = 0
        neg = np.stack(np.nonzero(adj), axis=0)
        neg[:, np.random.choice(neg.shape[1], samples, replace=True)].astype(np.int32)
        dense_ms = round((time.perf_counter() - t0) * 1e3, 3)
    emit(dict(kind="sampler", nodes=n, graph_edges=graph_edges, samples=samples, adjacency_build_ms=round(build_ms, 3),
              pairs_ms=stats(t_pairs), pairs_msamples_per_s=round(samples / float(np.median(t_pairs)) / 1e3, 2),
              start_node_ms=stats(t_from), start_node_msamples_per_s=round(samples / float(np.median(t_from)) / 1e3, 2),
              dense_ms=dense_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2449029)
    ap.add_argument("--edges", type=int, default=123718280)
    ap.add_argument("--features", default="16,100,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-chunk", type=int, default=1 << 23)
    ap.add_argument("--ceiling-glines", type=float, default=49.4)
    ap.add_argument("--sampler-edges", type=int, default=None)
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--dense-sizes", default="2000,8000")
    ap.add_argument("--dense-limit-bytes", type=int, default=4 << 30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = tfg._lib.device()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for F in [int(f) for f in args.features.split(",") if f]:
        bench_edge_dot(args.nodes, args.edges, F, args.rounds, args.torch_chunk, args.ceiling_glines, dev, emit)
        torch.cuda.empty_cache()
    bench_sampler(args.nodes, args.sampler_edges or args.edges, args.samples, args.rounds, args.dense_limit_bytes, dev, emit)
    for n in [int(s) for s in args.dense_sizes.split(",") if s]:
        bench_sampler(n, 8 * n, min(args.samples, 1 << 16), args.rounds, args.dense_limit_bytes, dev, emit)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
