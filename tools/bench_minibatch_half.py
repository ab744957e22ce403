# coding=utf-8
"""The minibatch route over a float32 feature table against the same table kept in 16 bits (prepare_half_features(...,
minibatch=True): bf16 and fp16 on the line-friendly stride, include/tfgx_minibatch_h16.h), on uniform and R-MAT graphs
(tf_geometric_amd.synthetic) at the ogbn-products shape (N = 2.4 M, E = 123 M); 1024 seeds, fanouts = [25, 10], F = 100, layer 0 =
MeanGraphSage(256).  Per table:

  (K) kernel  : sample_reduce alone on pre-drawn destination rows (tfgx_samplereduce_f32 / tfgx_sample_reduce_h16);
  (F) forward : sample_blocks(fuse_input_hop=True) + gather + input_aggregate + layer.combine, no grad;
  (S) step    : the same with the backward to the layer's weights;
  (R) replay  : one replay of a captured two-layer training step (CapturedTrainStep over sample_blocks_static(fuse_input_hop=True),
                gather, input_aggregate, both layers, the masked loss, backward, Adam).

The float32 rows are the route as it was before 16-bit tables reached it (its kernels compile to the same code): the baseline.
The table bytes are derived, not measured: N * F * 4 against N * h16_friendly_ld(F) * 2.

Method (tools/bench_input_hop.py's): a host clock around work that ends in a device synchronise; the tables alternate call by
call in one process after a warm-up, on the same pre-drawn seed batches; the whole comparison is repeated (--repeats) and the
spread between the repeats' medians is reported.  A table counts as ahead only when its median is below float32's by more than the
larger spread.  There is no threshold: the numbers are the result.

    python tools/bench_minibatch_half.py [--out profiles/minibatch_half_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = ("float32", "bf16", "fp16")
MEASURES = ("kernel", "forward", "step", "replay")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=2400000)
    p.add_argument("--edges", type=int, default=123000000)
    p.add_argument("--graphs", nargs="+", default=["uniform", "rmat"])
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", type=int, nargs="+", default=[25, 10])
    p.add_argument("--features", type=int, default=100)
    p.add_argument("--units", type=int, default=256)
    p.add_argument("--calls", type=int, default=30, help="timed calls per table and repeat")
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd.plan import h16_friendly_ld
    from tf_geometric_amd.synthetic import rmat_edges, synthetic_edges
    assert torch.cuda.is_available(), "bench_minibatch_half needs a GPU: there is nothing to time without one"
    dev = L.device()
    N, fanouts, F = args.nodes, list(args.fanouts), args.features
    rng = np.random.Generator(np.random.PCG64(7))
    x = torch.from_numpy(rng.standard_normal((N, F), dtype=np.float32)).to(dev)
    tables = {"float32": x, "bf16": tfg.prepare_half_features(x, torch.bfloat16, minibatch=True),
              "fp16": tfg.prepare_half_features(x, torch.float16, minibatch=True)}
    table_bytes = {"float32": N * F * 4, "bf16": N * h16_friendly_ld(F) * 2, "fp16": N * h16_friendly_ld(F) * 2}
    layer = tfg.layers.MeanGraphSage(args.units, activation=tfg.relu, concat=True).trainable(True)
    layer._maybe_build([x])
    params = [layer.self_kernel, layer.neighbor_kernel, layer.bias]

    def kernel(sampler, batch, call_seed, table):
        return tfg.utils.minibatch.sample_reduce(sampler, batch["rows"], table, fanouts[0], op="mean", seed=call_seed, _own_ids=True)

    def layer0(sampler, batch, call_seed, table):
        mb = sampler.sample_blocks(batch["seeds"], fanouts, seed=call_seed, fuse_input_hop=True)
        return layer.combine([mb.gather(table), mb.input_aggregate(table, "mean")], training=True)

    def forward(sampler, batch, call_seed, table):
        with torch.no_grad():
            return layer0(sampler, batch, call_seed, table)

    def step(sampler, batch, call_seed, table):
        for q in params:
            q.grad = None
        out = layer0(sampler, batch, call_seed, table)
        out.sum().backward()
        return out

    def captured_steps(sampler, seeds_buf):
        """One captured two-layer training step per table, each over layers and a seed word of its own."""
        steps = {}
        for name in TABLES:
            table = tables[name]
            layers = [tfg.layers.MeanGraphSage(args.units, activation=tfg.relu, concat=True).trainable(True),
                      tfg.layers.MeanGraphSage(64, activation=None, concat=True).trainable(True)]
            layers[0]._maybe_build([x])
            layers[1]._maybe_build([torch.empty(1, args.units)])
            opt = torch.optim.Adam([q for s in layers for q in s.parameters()], lr=1e-3, capturable=True)
            state = torch.full((1,), 777, dtype=torch.int64, device=dev)

            def loss_fn(table=table, layers=layers, state=state):
                mb = sampler.sample_blocks_static(seeds_buf, fanouts, seed=state, fuse_input_hop=True)
                state.add_(1)
                h = layers[0].combine([mb.gather(table), mb.input_aggregate(table, "mean")], training=True)
                b = mb.blocks[0]
                h = layers[1]([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
                return ((h[:args.seeds] ** 2).sum(1) * mb.seed_mask).sum() / mb.seed_mask.sum().clamp(min=1)

            steps[name] = tfg.CapturedTrainStep(loss_fn, opt)
        return steps

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    result = {"nodes": N, "seeds": args.seeds, "fanouts": fanouts, "features": F, "units": args.units, "calls": args.calls,
              "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "table_bytes_derived": table_bytes,
              "row_stride_elements": {"float32": F, "bf16": h16_friendly_ld(F), "fp16": h16_friendly_ld(F)},
              "method": "host clock around work ending in a device synchronise; tables alternate call by call; ms", "graphs": {}}
    for kind in args.graphs:
        E = args.edges
        ei = rmat_edges(N, E, 0, dev) if kind == "rmat" else torch.from_numpy(synthetic_edges(N, E, seed=0)).to(dev)
        sampler = tfg.utils.RandomNeighborSampler(ei)
        e_real = int(ei.shape[1])
        del ei
        batches = []
        for i in range(args.warmup + args.calls):
            seeds = torch.from_numpy(rng.choice(N, args.seeds, replace=False))
            rows = sampler.sample_blocks(seeds, fanouts, seed=50 + i, fuse_input_hop=True).node_index
            batches.append({"seeds": seeds, "rows": rows, "seeds_dev": seeds.to(dev, torch.int32)})
        # the contract, once per graph at the size that is timed: a 16-bit table gives the float32 route's bits on its widened copy
        bits = {}
        for name in ("bf16", "fp16"):
            got = kernel(sampler, batches[0], 9, tables[name])
            bits[name] = bool(torch.equal(got, kernel(sampler, batches[0], 9, tables[name].float())))
        seeds_buf = batches[0]["seeds_dev"].clone()
        replays = captured_steps(sampler, seeds_buf)

        def replay(sampler_, batch, call_seed, name):
            seeds_buf.copy_(batch["seeds_dev"])
            return replays[name]()

        routes = [(m, name) for m in MEASURES for name in TABLES]
        fns = {"kernel": kernel, "forward": forward, "step": step}

        def call(measure, name, batch, call_seed):
            if measure == "replay":
                return timed(replay, sampler, batch, call_seed, name)[0]
            return timed(fns[measure], sampler, batch, call_seed, tables[name])[0]

        for i in range(args.warmup):
            for measure, name in routes:
                call(measure, name, batches[i], 100 + i)
        medians = {r: [] for r in routes}
        for rep in range(args.repeats):
            t = {r: [] for r in routes}
            for i in range(args.warmup, args.warmup + args.calls):
                for r in routes:
                    t[r].append(call(r[0], r[1], batches[i], 1000 * rep + i))
            for r in routes:
                medians[r].append(float(np.median(t[r])))
        entry = {"edges": e_real, "mean_rows": float(np.mean([b["rows"].numel() for b in batches])),
                 "h16_equals_float32_on_widened_table": bits, "measures": {}}
        for measure in MEASURES:
            med = {name: float(np.median(medians[(measure, name)])) for name in TABLES}
            spread = {name: float(max(medians[(measure, name)]) - min(medians[(measure, name)])) for name in TABLES}
            cmp = {}
            for name in ("bf16", "fp16"):
                bar = max(spread[name], spread["float32"])
                gap = med["float32"] - med[name]
                cmp[name + "_vs_float32"] = {"gap_ms": gap, "larger_spread_ms": bar, "ahead_beyond_spread": bool(gap > bar),
                                             "behind_beyond_spread": bool(-gap > bar), "ratio": med["float32"] / med[name]}
            entry["measures"][measure] = {"median_ms": med, "spread_ms": spread,
                                          "repeat_medians_ms": {name: medians[(measure, name)] for name in TABLES}, "comparisons": cmp}
            print("{:8s} E = {:>11d} {:8s}: ".format(kind, e_real, measure) + "  ".join(
                "{} {:.3f} (+-{:.3f})".format(name, med[name], spread[name]) for name in TABLES) + "  ahead: " + ", ".join(
                "{} {}".format(name, cmp[name + "_vs_float32"]["ahead_beyond_spread"]) for name in ("bf16", "fp16")), flush=True)
        result["graphs"][kind] = entry
        if args.out:                         # after every graph: a run cut short keeps what it measured
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
        del sampler, batches, replays
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
