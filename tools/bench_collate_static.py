# coding=utf-8
"""One whole training step of examples/demo_mean_pool.py (GCN(64) -> GCN(32) -> mean readout -> dense, Adam) on its dataset
(4000 graphs of 10-50 nodes, F = 37), batches of 128 and 512 graphs, three ways:

  (A) collate          : GraphStore.collate of host-drawn ids, the step issued launch by launch   (the route of `batches`)
  (B) collate_static   : StaticLoader.next_ids + GraphStore.collate_static at worst-case capacities, issued launch by launch
  (C) replayed         : (B) recorded once by tfg.CapturedTrainStep and replayed from one hipGraph

and batch assembly alone, collate against next_ids + collate_static.

Method (that of tools/bench_collate.py): a host clock around work that ends in a device synchronise; the variants alternate
step by step in one process, after a warm-up; the whole comparison is repeated (--repeats) so the spread between the repeats'
medians is known.  (C) counts as ahead of (A) only when its median is below (A)'s by more than the SUM of the two spreads.
Each variant trains a model of its own (the time of a step does not depend on the weights).  Not measured here: where inside
a step the time goes (no kernel trace), and the cost of the padded rows by itself — only their share, n_cap / n_live, is
reported, read from the batches' `counts`.

    python tools/bench_collate_static.py [--out profiles/collate_static_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--batch-sizes", type=int, nargs="+", default=[128, 512])
    p.add_argument("--steps", type=int, default=60, help="timed steps per variant and repeat (at least 50)")
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from demo_mean_pool import MeanPoolNetwork, batch_loss, make_static_loss_fn
    from demo_sag_pool_h import make_dataset
    from demo_graph_store import to_graphs
    assert torch.cuda.is_available(), "bench_collate_static needs a GPU: there is nothing to time without one"

    data = make_dataset(args.graphs, 0)
    store = tfg.data.GraphStore(to_graphs(data, range(len(data.graphs))))
    F, G = store.num_features, len(store)
    rng = np.random.Generator(np.random.PCG64(7))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def summary(medians):
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
        return {"median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread}

    result = {"dataset": {"graphs": G, "nodes": int(store.node_ptr[-1]), "edges": int(store.edge_ptr[-1]), "F": F},
              "method": "host clock around work ending in a device synchronise; variants alternate step by step; ms",
              "batch_sizes": {}}
    for bs in args.batch_sizes:
        cap = store.static_capacities(bs)
        torch.manual_seed(0)

        def eager_step(model, opt, make_batch):
            def step():
                opt.zero_grad(set_to_none=True)
                loss = batch_loss(model, make_batch())
                loss.backward()
                opt.step()
                return loss
            return step

        pool = [rng.choice(G, bs, replace=False) for _ in range(256)]       # drawn ahead, as `batches` draws its epoch order ahead
        turn = iter(range(1 << 30))

        def host_ids():
            return pool[next(turn) % len(pool)]

        model_a, model_b, model_c = (MeanPoolNetwork(F, 2, seed=0) for _ in range(3))
        loader_b = store.static_loader(bs, shuffle=True, seed=1)
        loader_c = store.static_loader(bs, shuffle=True, seed=1)
        steps = {"collate": eager_step(model_a, torch.optim.Adam(model_a.parameters(), lr=5e-3), lambda: store.collate(host_ids())),
                 "collate_static": eager_step(model_b, torch.optim.Adam(model_b.parameters(), lr=5e-3),
                                              lambda: store.collate_static(loader_b.next_ids(), cap)),
                 "replayed": tfg.CapturedTrainStep(make_static_loss_fn(model_c, store, loader_c, cap),
                                                   torch.optim.Adam(model_c.parameters(), lr=5e-3, capturable=True))}
        alone = {"collate": lambda: store.collate(host_ids()),
                 "collate_static": lambda: store.collate_static(loader_b.next_ids(), cap)}
        entry = {"capacities": cap._asdict()}
        for what, variants in (("step", steps), ("assembly_alone", alone)):
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            medians = {k: [] for k in variants}
            for _ in range(args.repeats):
                t = {k: [] for k in variants}
                for _ in range(max(args.steps, 50)):
                    for k, fn in variants.items():
                        t[k].append(timed(fn)[0])
                for k in t:
                    medians[k].append(float(np.median(t[k])))
            entry[what] = summary(medians)
        s = entry["step"]
        gap = s["median_ms"]["collate"] - s["median_ms"]["replayed"]
        entry["replayed_ahead_of_collate_beyond_spreads"] = bool(gap > s["spread_ms"]["collate"] + s["spread_ms"]["replayed"])
        # the share of padding, from the batches' own counts (one epoch of the loader's batches)
        loader_b.cursor.zero_()
        counts = torch.stack([store.collate_static(loader_b.next_ids(), cap).counts for _ in range(loader_b.steps_per_epoch)])
        counts = counts.cpu().numpy().astype(np.float64)
        full = counts[:, 0] == bs
        entry["padding"] = {"n_cap": cap.n_cap, "e_cap": cap.e_cap, "mean_n_live_full_batches": float(counts[full, 1].mean()),
                            "mean_e_live_full_batches": float(counts[full, 2].mean()),
                            "n_cap_over_n_live": float(cap.n_cap / counts[full, 1].mean()),
                            "e_cap_over_e_live": float(cap.e_cap / counts[full, 2].mean())}
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: step  collate {:.3f}  collate_static {:.3f}  replayed {:.3f} ms  (spreads {:.3f} / {:.3f} / {:.3f})  "
              "replayed ahead beyond spreads: {}".format(bs, *(s["median_ms"][k] for k in steps), *(s["spread_ms"][k] for k in steps),
                                                         entry["replayed_ahead_of_collate_beyond_spreads"]), flush=True)
        a = entry["assembly_alone"]
        print("            alone collate {:.3f}  next_ids + collate_static {:.3f} ms  (spreads {:.3f} / {:.3f})  n_cap / n_live {:.2f}".format(
            a["median_ms"]["collate"], a["median_ms"]["collate_static"], a["spread_ms"]["collate"], a["spread_ms"]["collate_static"],
            entry["padding"]["n_cap_over_n_live"]), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
