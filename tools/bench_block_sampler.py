# coding=utf-8
"""A sampled 2-hop minibatch ready for two layers, two ways, on uniform and R-MAT graphs (tf_geometric_amd.synthetic) at the
ogbn-products shape (N = 2.4 M, E = 123 M) and at a tenth of its edges; 1024 seeds, fanouts = [25, 10]:

  (A) blocks : RandomNeighborSampler.sample_blocks — per hop the row-list sampler and the order-stable relabel, plans attached;
  (B) parent : what the package offered before — per hop sample(k, sampled_node_index=(rows, arange(N))) (the virtual
               sub-graph of the listed rows: passes over every edge of the graph), torch.unique plus an N-sized index map for
               the relabel, and no attached plan, so the plan build of the first layer call (CsrPlan.build) is counted.

Both produce, per layer, a relabelled edge list over the seeds' sampled neighbourhood (B numbers the new nodes in sorted
order and draws from a generator keyed by list position, so the two samples differ in their draws, not in their kind).

Method: a host clock around work that ends in a device synchronise; the two routes alternate call by call in one process after
a warm-up, on the same pre-drawn seed batches; the whole comparison is repeated (--repeats) and the spread between the
repeats' medians is reported.  (A) counts as ahead only when its median is below (B)'s by more than the larger spread; (A) counts
as independent of E when its medians at the two edge counts differ by no more than the larger spread.  For (A) the hop next to
the seeds is also timed alone (fanouts = [10]); the outer hop is the difference.  Host synchronisations of (A) are the reads
sample_blocks counts itself (SampledMinibatch.num_host_syncs).

    python tools/bench_block_sampler.py [--out profiles/block_sampler_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=2400000)
    p.add_argument("--edges", type=int, nargs="+", default=[123000000, 12300000])
    p.add_argument("--graphs", nargs="+", default=["uniform", "rmat"])
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", type=int, nargs="+", default=[25, 10])
    p.add_argument("--calls", type=int, default=30, help="timed calls per route and repeat")
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd.plan import CsrPlan
    from tf_geometric_amd.synthetic import rmat_edges, synthetic_edges
    assert torch.cuda.is_available(), "bench_block_sampler needs a GPU: there is nothing to time without one"
    dev = tfg._lib.device()
    N, fanouts = args.nodes, list(args.fanouts)
    rng = np.random.Generator(np.random.PCG64(7))

    def route_a(sampler, seeds, call_seed):
        mb = sampler.sample_blocks(seeds, fanouts, seed=call_seed)
        return mb, mb.node_index.numel(), sum(b.num_edges for b in mb.blocks)

    def route_a_inner(sampler, seeds, call_seed):
        mb = sampler.sample_blocks(seeds, fanouts[-1:], seed=call_seed)
        return mb, mb.node_index.numel(), mb.blocks[0].num_edges

    def route_b(sampler, seeds, call_seed):
        every = torch.arange(N, dtype=torch.int32, device=dev)
        node_index = seeds.to(dev).long()
        blocks, edges = [], 0
        for h in range(len(fanouts)):
            ei, ew = sampler.sample(k=fanouts[len(fanouts) - 1 - h], sampled_node_index=(node_index.to(torch.int32), every),
                                    seed=call_seed + h)
            cols = ei[1].long()
            known = torch.zeros(N, dtype=torch.bool, device=dev)
            known[node_index] = True
            node_index = torch.cat([node_index, torch.unique(cols[~known[cols]])])
            index_map = torch.full((N,), -1, dtype=torch.int32, device=dev)
            index_map[node_index] = torch.arange(node_index.shape[0], dtype=torch.int32, device=dev)
            block = torch.stack([ei[0], index_map[cols]])
            n_src = int(node_index.shape[0])
            CsrPlan.build(block, n_src, n_src)            # the sort the first layer call pays without an attached plan
            blocks.append((block, ew))
            edges += int(block.shape[1])
        return blocks, int(node_index.shape[0]), edges

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    result = {"nodes": N, "seeds": args.seeds, "fanouts": fanouts, "calls": args.calls, "repeats": args.repeats,
              "method": "host clock around work ending in a device synchronise; routes alternate call by call; ms",
              "device": torch.cuda.get_device_name(0), "graphs": {}}
    routes = (("blocks", route_a), ("blocks_inner_hop", route_a_inner), ("parent", route_b))
    for kind in args.graphs:
        for E in args.edges:
            ei = rmat_edges(N, E, 0, dev) if kind == "rmat" else torch.from_numpy(synthetic_edges(N, E, seed=0)).to(dev)
            sampler = tfg.utils.RandomNeighborSampler(ei)
            e_real = int(ei.shape[1])
            del ei
            batches = [torch.from_numpy(rng.choice(N, args.seeds, replace=False)) for _ in range(args.warmup + args.calls)]
            for i in range(args.warmup):
                for _, fn in routes:
                    fn(sampler, batches[i], 100 + i)
            medians = {name: [] for name, _ in routes}
            sizes, syncs = {name: [] for name, _ in routes}, []
            for rep in range(args.repeats):
                t = {name: [] for name, _ in routes}
                for i in range(args.warmup, args.warmup + args.calls):
                    for name, fn in routes:
                        ms, out = timed(fn, sampler, batches[i], 1000 * rep + i)
                        t[name].append(ms)
                        sizes[name].append(out[1:])
                        if name == "blocks":
                            syncs.append(out[0].num_host_syncs)
                for name in t:
                    medians[name].append(float(np.median(t[name])))
            med = {k: float(np.median(v)) for k, v in medians.items()}
            spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
            entry = {"edges": e_real, "median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread,
                     "blocks_outer_hop_ms": med["blocks"] - med["blocks_inner_hop"],
                     "blocks_host_syncs": sorted(set(syncs)),
                     "mean_nodes": {k: float(np.mean([s[0] for s in v])) for k, v in sizes.items()},
                     "mean_edges": {k: float(np.mean([s[1] for s in v])) for k, v in sizes.items()},
                     "blocks_ahead_beyond_spread": bool(med["parent"] - med["blocks"] > max(spread["parent"], spread["blocks"])),
                     "parent_over_blocks": med["parent"] / med["blocks"]}
            result["graphs"]["{}_{}".format(kind, E)] = entry
            print("{:8s} E = {:>11d}: blocks {:.3f} ms (inner hop alone {:.3f}; spread {:.3f})  parent {:.3f} ms (spread {:.3f})  "
                  "ahead beyond spread: {}  syncs {}".format(kind, e_real, med["blocks"], med["blocks_inner_hop"], spread["blocks"],
                                                            med["parent"], spread["parent"], entry["blocks_ahead_beyond_spread"],
                                                            entry["blocks_host_syncs"]), flush=True)
            del sampler
            torch.cuda.empty_cache()
        if len(args.edges) >= 2:
            big, small = (result["graphs"]["{}_{}".format(kind, E)] for E in (max(args.edges), min(args.edges)))
            gap = abs(big["median_ms"]["blocks"] - small["median_ms"]["blocks"])
            bar = max(big["spread_ms"]["blocks"], small["spread_ms"]["blocks"])
            result["graphs"]["{}_blocks_time_independent_of_E".format(kind)] = {"gap_ms": gap, "larger_spread_ms": bar,
                                                                               "within_spread": bool(gap <= bar)}
            print("{:8s} blocks at E = {} vs {}: gap {:.3f} ms, larger spread {:.3f} ms".format(
                kind, max(args.edges), min(args.edges), gap, bar), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
