# coding=utf-8
"""Getting a minibatch of whole graphs ready for a forward + backward pass, two ways, on the dataset of
examples/demo_sag_pool_h.py (4000 graphs of 10-50 nodes, F = 37), batches of 128 and 512 graphs:

  (A) host      : make_batch (a Python loop over the graphs, numpy concatenation, five host-to-device copies), then what the
                  first training step pays on top: CsrPlan.build, plan.transposed() and the readouts' graph plan (three sorts,
                  each with its host synchronisation);
  (B) collate   : GraphStore.collate — one table copy and one kernel launch, the three plans included.

Method: a host clock around work that ends in a device synchronise; both variants alternate batch by batch in one process,
after a warm-up, on the same pre-drawn graph ids; the whole comparison is repeated (--repeats) so the spread between repeats
is known.  (B) counts as ahead only when its median is below (A)'s by more than that spread.  The demo's training step
(batch assembly included) is timed both ways in the same alternating manner.  The bytes the kernel moves are computed from
the batch's shapes.

    python tools/bench_collate.py [--out profiles/collate_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/bench_collate.py --trace-calls 97
    python tools/bench_collate.py --parse-trace <dir> --trace-calls 97      # launches per collate call, from that trace
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def kernel_bytes(B, n, e, F):
    """Bytes one collate call reads plus writes, from shapes: feature rows once in and once out; per edge the list (row, col,
    weight) and two plans' (col, perm) in, and those plus edge_graph_index out; per node node_graph_index out and two row_ptr
    entries in and out; the table in.  The slot lookups run on LDS (or on a cache-resident B + 1 offsets)."""
    return 2 * 4 * n * F + 4 * e * (7 + 8) + 4 * n * (1 + 2 + 2) + 4 * 4 * (B + 1)


def parse_trace(directory, calls):
    counts = {}
    for fn in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        with open(fn) as fh:
            for r in csv.DictReader(fh):
                counts[r["Kernel_Name"]] = counts.get(r["Kernel_Name"], 0) + 1
    def short(name):
        return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]

    merged = {}
    for k, v in counts.items():
        merged[short(k)] = merged.get(short(k), 0) + v
    # the run makes `calls` collate calls and nothing else that often (building the store sorts twice): a kernel launched at
    # least `calls` times belongs to the calls, and what is left over (`setup_launches`) to the set-up.  The table's
    # host-to-device copy shows up as the runtime's copy kernel.
    per_call = {k: v // calls for k, v in merged.items() if v >= calls}
    return {"trace_calls": calls, "launches_per_collate": per_call, "launches_per_collate_total": sum(per_call.values()),
            "setup_launches": {k: v - calls * per_call.get(k, 0) for k, v in sorted(merged.items()) if v - calls * per_call.get(k, 0)}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--batch-sizes", type=int, nargs="+", default=[128, 512])
    p.add_argument("--batches", type=int, default=60, help="timed batches per variant and repeat (at least 50)")
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--demo-steps", type=int, default=40, help="timed training steps per variant (0: skip)")
    p.add_argument("--trace-calls", type=int, default=0, help="only make this many collate calls (for a kernel trace)")
    p.add_argument("--parse-trace", default=None, help="directory of a rocprofv3 --kernel-trace run made with --trace-calls")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.parse_trace:
        result = parse_trace(args.parse_trace, args.trace_calls)
        print(json.dumps(result))
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
        return

    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd.plan import CsrPlan
    from tf_geometric_amd.nn.pool.common_pool import _graph_plan
    from demo_sag_pool_h import SAGPoolHModel, make_batch, make_dataset, train_step
    from demo_graph_store import as_inputs, to_graphs
    assert torch.cuda.is_available(), "bench_collate needs a GPU: there is nothing to time without one"

    data = make_dataset(args.graphs, 0)
    store = tfg.data.GraphStore(to_graphs(data, range(len(data.graphs))))
    F = store.num_features
    rng = np.random.Generator(np.random.PCG64(7))

    def draw(batch_size, count):
        return [rng.choice(len(store), batch_size, replace=False) for _ in range(count)]

    def host_ready(ids):
        x, ei, gid, y, num_graphs = make_batch(data, list(ids))
        n = int(x.shape[0])
        plan = CsrPlan.build(ei, n, n)
        plan.transposed()
        _graph_plan(gid, num_graphs, n, {})
        return x, ei, gid, y, num_graphs

    def collate_ready(ids):
        return as_inputs(store.collate(ids))

    def timed(fn, ids):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(ids)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if args.trace_calls:
        for ids in draw(512, args.trace_calls):
            store.collate(ids)
        torch.cuda.synchronize()
        print("made {} collate calls".format(args.trace_calls))
        return

    result = {"dataset": {"graphs": len(store), "nodes": int(store.node_ptr[-1]), "edges": int(store.edge_ptr[-1]), "F": F},
              "method": "host clock around work ending in a device synchronise; variants alternate batch by batch; ms",
              "batch_sizes": {}}
    for bs in args.batch_sizes:
        for ids in draw(bs, args.warmup):
            host_ready(ids)
            collate_ready(ids)
        medians = {"host": [], "collate": []}
        shapes = []
        for _ in range(args.repeats):
            t = {"host": [], "collate": []}
            for ids in draw(bs, max(args.batches, 50)):
                ms_a, a = timed(host_ready, ids)
                ms_b, b = timed(collate_ready, ids)
                t["host"].append(ms_a)
                t["collate"].append(ms_b)
                shapes.append((int(b[0].shape[0]), int(b[1].shape[1])))
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
            for k in t:
                medians[k].append(float(np.median(t[k])))
        n_mean, e_mean = (float(np.mean([s[i] for s in shapes])) for i in (0, 1))
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
        entry = {"median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread,
                 "collate_ahead_beyond_spread": bool(med["host"] - med["collate"] > max(spread.values())),
                 "host_over_collate": med["host"] / med["collate"], "mean_nodes": n_mean, "mean_edges": e_mean,
                 "kernel_bytes_per_batch": int(kernel_bytes(bs, n_mean, e_mean, F))}
        if args.demo_steps:
            torch.manual_seed(0)
            model = SAGPoolHModel(F, 2, seed=0)
            opt = torch.optim.Adam(model.parameters(), lr=5e-4)
            steps = {"host": [], "collate": []}
            for i, ids in enumerate(draw(bs, args.warmup + args.demo_steps)):
                for name, fn in (("host", lambda ids: make_batch(data, list(ids))), ("collate", collate_ready)):
                    ms, _ = timed(lambda ids: train_step(model, opt, fn(ids)), ids)
                    if i >= args.warmup:
                        steps[name].append(ms)
            entry["demo_ms_per_step"] = {k: float(np.median(v)) for k, v in steps.items()}
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: host {:.3f} ms  collate {:.3f} ms  (spread {:.3f} / {:.3f})  ahead beyond spread: {}  demo step {}".format(
            bs, med["host"], med["collate"], spread["host"], spread["collate"], entry["collate_ahead_beyond_spread"],
            entry.get("demo_ms_per_step")), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
