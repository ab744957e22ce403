# coding=utf-8
"""The input hop of a sampled minibatch, fused against unfused, on uniform and R-MAT graphs (tf_geometric_amd.synthetic) at the
ogbn-products shape (N = 2.4 M, E = 123 M) and at a tenth of its edges; 1024 seeds, fanouts = [25, 10], F = 100, layer 0 =
MeanGraphSage(256):

  (A) fused   : sample_blocks(fuse_input_hop=True) + gather + input_aggregate (tfgx_samplereduce_f32: the hop drawn and reduced
                out of the global table in one launch) + layer.combine on the n_1 destination rows;
  (B) unfused : sample_blocks + gather of all n_2 rows + the layer over blocks[0], [:num_dst] kept — the route as it was.

Each as a forward pass (no grad) and as forward + backward (d/d weights of the layer's summed output).  Also the kernel's job
alone, on the same pre-drawn destination rows: (K) sample_reduce against (S) sample_rows' kernels + relabel + gather_rows +
segment_reduce (sample_blocks over one hop, gather, the reduction over the block's attached plan).

Method: a host clock around work that ends in a device synchronise; the routes alternate call by call in one process after a
warm-up, on the same pre-drawn seed batches; the whole comparison is repeated (--repeats) and the spread between the repeats'
medians is reported.  A route counts as ahead only when its median is below the other's by more than the larger spread.

    python tools/bench_input_hop.py [--out profiles/input_hop_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = (("fused_forward", "unfused_forward"), ("fused_step", "unfused_step"), ("kernel_fused", "kernel_composed"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=2400000)
    p.add_argument("--edges", type=int, nargs="+", default=[123000000, 12300000])
    p.add_argument("--graphs", nargs="+", default=["uniform", "rmat"])
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", type=int, nargs="+", default=[25, 10])
    p.add_argument("--features", type=int, default=100)
    p.add_argument("--units", type=int, default=256)
    p.add_argument("--calls", type=int, default=30, help="timed calls per route and repeat")
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd.plan import attached_plan, segment_reduce
    from tf_geometric_amd.synthetic import rmat_edges, synthetic_edges
    assert torch.cuda.is_available(), "bench_input_hop needs a GPU: there is nothing to time without one"
    dev = L.device()
    N, fanouts, F = args.nodes, list(args.fanouts), args.features
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy(rng.standard_normal((N, F), dtype=np.float32)).to(dev)
    layer = tfg.layers.MeanGraphSage(args.units, activation=tfg.relu, concat=True).trainable(True)
    layer._maybe_build([x])
    params = [layer.self_kernel, layer.neighbor_kernel, layer.bias]

    def fused(sampler, seeds, call_seed):
        mb = sampler.sample_blocks(seeds, fanouts, seed=call_seed, fuse_input_hop=True)
        return layer.combine([mb.gather(x), mb.input_aggregate(x, "mean")], training=True), mb.node_index.numel(), 0

    def unfused(sampler, seeds, call_seed):
        mb = sampler.sample_blocks(seeds, fanouts, seed=call_seed)
        b = mb.blocks[0]
        h = layer([mb.gather(x)[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        return h, mb.node_index.numel(), b.num_edges

    def forward(route):
        def run(sampler, batch, call_seed):
            with torch.no_grad():
                return route(sampler, batch["seeds"], call_seed)
        return run

    def step(route):
        def run(sampler, batch, call_seed):
            for q in params:
                q.grad = None
            out = route(sampler, batch["seeds"], call_seed)
            out[0].sum().backward()
            return out
        return run

    def kernel_fused(sampler, batch, call_seed):
        out = tfg.utils.minibatch.sample_reduce(sampler, batch["rows"], x, fanouts[0], op="mean", seed=call_seed, _own_ids=True)
        return out, batch["rows"].numel(), 0

    def kernel_composed(sampler, batch, call_seed):
        mb = sampler.sample_blocks(batch["rows"], fanouts[:1], seed=call_seed)
        b = mb.blocks[0]
        out = segment_reduce(attached_plan(b.edge_index), mb.gather(x), L.MEAN, w_csr=b.edge_weight)
        return out, mb.node_index.numel(), b.num_edges

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    routes = (("fused_forward", forward(fused)), ("unfused_forward", forward(unfused)), ("fused_step", step(fused)),
              ("unfused_step", step(unfused)), ("kernel_fused", kernel_fused), ("kernel_composed", kernel_composed))
    result = {"nodes": N, "seeds": args.seeds, "fanouts": fanouts, "features": F, "units": args.units, "calls": args.calls,
              "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "method": "host clock around work ending in a device synchronise; routes alternate call by call; ms", "graphs": {}}
    for kind in args.graphs:
        for E in args.edges:
            ei = rmat_edges(N, E, 0, dev) if kind == "rmat" else torch.from_numpy(synthetic_edges(N, E, seed=0)).to(dev)
            sampler = tfg.utils.RandomNeighborSampler(ei)
            e_real = int(ei.shape[1])
            del ei
            batches = []
            for i in range(args.warmup + args.calls):
                seeds = torch.from_numpy(rng.choice(N, args.seeds, replace=False))
                rows = sampler.sample_blocks(seeds, fanouts, seed=50 + i, fuse_input_hop=True).node_index
                batches.append({"seeds": seeds, "rows": rows})
            # the two routes compute the same thing: compared once per graph at the size that is timed (same seed, same draws)
            with torch.no_grad():
                a, b = fused(sampler, batches[0]["seeds"], 9)[0], unfused(sampler, batches[0]["seeds"], 9)[0]
            agree = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
            for i in range(args.warmup):
                for _, fn in routes:
                    fn(sampler, batches[i], 100 + i)
            medians = {name: [] for name, _ in routes}
            sizes = {name: [] for name, _ in routes}
            for rep in range(args.repeats):
                t = {name: [] for name, _ in routes}
                for i in range(args.warmup, args.warmup + args.calls):
                    for name, fn in routes:
                        ms, out = timed(fn, sampler, batches[i], 1000 * rep + i)
                        t[name].append(ms)
                        sizes[name].append(out[1:])
                for name in t:
                    medians[name].append(float(np.median(t[name])))
            med = {k: float(np.median(v)) for k, v in medians.items()}
            spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
            entry = {"edges": e_real, "median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread,
                     "mean_nodes": {k: float(np.mean([s[0] for s in v])) for k, v in sizes.items()},
                     "mean_edges": {k: float(np.mean([s[1] for s in v])) for k, v in sizes.items()},
                     "fused_vs_unfused_forward_max_rel_diff": agree, "comparisons": {}}
            for new, old in PAIRS:
                bar = max(spread[new], spread[old])
                entry["comparisons"][new + "_vs_" + old] = {
                    "gap_ms": med[old] - med[new], "larger_spread_ms": bar, "ahead_beyond_spread": bool(med[old] - med[new] > bar),
                    "ratio": med[old] / med[new]}
            result["graphs"]["{}_{}".format(kind, E)] = entry
            print("{:8s} E = {:>11d}: ".format(kind, e_real) + "  ".join(
                "{} {:.3f} (+-{:.3f}) vs {} {:.3f} (+-{:.3f}) ahead: {}".format(
                    new, med[new], spread[new], old, med[old], spread[old],
                    entry["comparisons"][new + "_vs_" + old]["ahead_beyond_spread"]) for new, old in PAIRS)
                + "  forward rel diff {:.2e}".format(agree), flush=True)
            del sampler, batches
            torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
