# coding=utf-8
"""A sampled minibatch and a whole training step, dynamic shapes against fixed shapes against a hipGraph replay, on uniform and
R-MAT graphs (tf_geometric_amd.synthetic) at the ogbn-products shape (N = 2.4 M, E = 123 M) and at a tenth of its edges; 1024
seeds, fanouts = [25, 10], F = 100, two layers of MeanGraphSage(256), Adam:

  (A) dynamic  : sample_blocks(fuse_input_hop=True) — L host reads per call; the best route before fixed shapes;
  (B) static   : sample_blocks_static(fuse_input_hop=True), eager — no host read, every tensor at its capacity;
  (C) captured : the same launch sequence replayed from a hipGraph (torch.cuda.CUDAGraph for the sample alone,
                 CapturedTrainStep for the step: sample -> forward -> backward -> Adam).

Each as the sample alone ("minibatch") and as a whole training step ("step").  Also the capacity waste of the fixed shapes: live
nodes and edges over capacity, hop by hop, from one unfused static sample per call batch.

Method (that of tools/bench_input_hop.py): a host clock around work that ends in a device synchronise; the routes alternate call
by call in one process after a warm-up, on the same pre-drawn seed batches; the whole comparison is repeated (--repeats) and the
spread between the repeats' medians is reported.  A route counts as ahead only when its median is below the other's by more than
the larger spread.

    python tools/bench_static_minibatch.py [--out profiles/static_minibatch_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = (("static_minibatch", "dynamic_minibatch"), ("captured_minibatch", "dynamic_minibatch"),
         ("static_step", "dynamic_step"), ("captured_step", "dynamic_step"))


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
    from tf_geometric_amd.synthetic import rmat_edges, synthetic_edges
    assert torch.cuda.is_available(), "bench_static_minibatch needs a GPU: there is nothing to time without one"
    dev = L.device()
    N, fanouts, F, B = args.nodes, list(args.fanouts), args.features, args.seeds
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy(rng.standard_normal((N, F), dtype=np.float32)).to(dev)

    def make_model():
        layers = [tfg.layers.MeanGraphSage(args.units, activation=tfg.relu, concat=True).trainable(True)
                  for _ in range(len(fanouts))]
        layers[0]._maybe_build([x])
        for layer in layers[1:]:
            layer._maybe_build([torch.empty(1, args.units)])
        opt = torch.optim.Adam([q for layer in layers for q in layer.parameters()], lr=1e-3, capturable=True)
        return layers, opt

    def model(layers, mb):
        h = layers[0].combine([mb.gather(x), mb.input_aggregate(x, "mean")], training=True)
        for layer, b in zip(layers[1:], mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        return h

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    cap = tfg.utils.static_capacities(B, fanouts)
    result = {"nodes": N, "seeds": B, "fanouts": fanouts, "features": F, "units": args.units, "calls": args.calls,
              "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "capacities": {"rows": cap.rows, "edges": cap.edges, "sinks": cap.sinks},
              "method": "host clock around work ending in a device synchronise; routes alternate call by call; ms", "graphs": {}}
    for kind in args.graphs:
        for E in args.edges:
            ei = rmat_edges(N, E, 0, dev) if kind == "rmat" else torch.from_numpy(synthetic_edges(N, E, seed=0)).to(dev)
            sampler = tfg.utils.RandomNeighborSampler(ei)
            e_real = int(ei.shape[1])
            del ei
            batches = [torch.from_numpy(rng.choice(N, B, replace=False)).to(torch.int32).to(dev)
                       for _ in range(args.warmup + args.calls)]
            seeds_buf = batches[0].clone()
            state = torch.full((1,), 1000, dtype=torch.int64, device=dev)
            layers_e, opt_e = make_model()          # the eager routes share one model
            layers_c, opt_c = make_model()          # the captured step owns its own (its gradients live in the graph's pool)

            def dynamic_minibatch(seeds, call_seed):
                return sampler.sample_blocks(seeds, fanouts, seed=call_seed, fuse_input_hop=True)

            def static_minibatch(seeds, call_seed):
                seeds_buf.copy_(seeds)
                mb = sampler.sample_blocks_static(seeds_buf, fanouts, seed=state, fuse_input_hop=True)
                state.add_(1)
                return mb

            def dynamic_step(seeds, call_seed):
                opt_e.zero_grad(set_to_none=True)
                mb = dynamic_minibatch(seeds, call_seed)
                model(layers_e, mb)[:mb.num_seeds].sum().backward()
                opt_e.step()

            def static_loss(layers):
                mb = sampler.sample_blocks_static(seeds_buf, fanouts, seed=state, fuse_input_hop=True)
                state.add_(1)
                return (model(layers, mb)[:B] * mb.seed_mask[:, None]).sum()

            def static_step(seeds, call_seed):
                seeds_buf.copy_(seeds)
                opt_e.zero_grad(set_to_none=True)
                static_loss(layers_e).backward()
                opt_e.step()

            static_minibatch(batches[0], 0)          # the sampler's state exists before any capture
            torch.cuda.synchronize()
            sample_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(sample_graph):
                captured_mb = sampler.sample_blocks_static(seeds_buf, fanouts, seed=state, fuse_input_hop=True)
                state.add_(1)
            train_graph = tfg.CapturedTrainStep(lambda: static_loss(layers_c), opt_c)

            def captured_minibatch(seeds, call_seed):
                seeds_buf.copy_(seeds)
                sample_graph.replay()

            def captured_step(seeds, call_seed):
                seeds_buf.copy_(seeds)
                train_graph()

            routes = (("dynamic_minibatch", dynamic_minibatch), ("static_minibatch", static_minibatch),
                      ("captured_minibatch", captured_minibatch), ("dynamic_step", dynamic_step), ("static_step", static_step),
                      ("captured_step", captured_step))
            # the three samplers draw the same minibatch: compared once per graph at the size that is timed
            seeds_buf.copy_(batches[0])
            state.fill_(77)
            sample_graph.replay()
            torch.cuda.synchronize()
            dyn = sampler.sample_blocks(batches[0], fanouts, seed=77, fuse_input_hop=True)
            same = bool(torch.equal(captured_mb.node_index[captured_mb.live], dyn.node_index))
            # capacity waste, both hops: one unfused static sample per batch, its device counts read afterwards
            waste = []
            for i, seeds in enumerate(batches[:8]):
                mb = sampler.sample_blocks_static(seeds, fanouts, seed=50 + i)
                waste.append((mb.counts.cpu().numpy(), int(mb.live.sum())))
            counts = np.mean([w[0] for w in waste], axis=0)
            capacity = {"edges_live_over_capacity": [float(counts[h, 0]) / max(cap.edges[h], 1) for h in range(len(fanouts))],
                        "new_nodes_live_over_slots": [float(counts[h, 1]) / max(cap.edges[h], 1) for h in range(len(fanouts))],
                        "mean_edges": [float(v) for v in counts[:, 0]], "mean_new_nodes": [float(v) for v in counts[:, 1]],
                        "live_nodes_over_capacity": float(np.mean([w[1] for w in waste])) / cap.rows[-1]}
            for i in range(args.warmup):
                for _, fn in routes:
                    fn(batches[i], 100 + i)
            medians = {name: [] for name, _ in routes}
            for rep in range(args.repeats):
                t = {name: [] for name, _ in routes}
                for i in range(args.warmup, args.warmup + args.calls):
                    for name, fn in routes:
                        t[name].append(timed(fn, batches[i], 1000 * rep + i))
                for name in t:
                    medians[name].append(float(np.median(t[name])))
            med = {k: float(np.median(v)) for k, v in medians.items()}
            spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
            entry = {"edges": e_real, "median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread,
                     "captured_sample_equals_dynamic": same, "capacity": capacity, "comparisons": {}}
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
                + "  same sample: {}  edges/capacity {}  live nodes/capacity {:.3f}".format(
                    same, ["{:.3f}".format(v) for v in capacity["edges_live_over_capacity"]], capacity["live_nodes_over_capacity"]),
                flush=True)
            del sampler, batches, sample_graph, train_graph, captured_mb, layers_e, layers_c, opt_e, opt_c
            torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
