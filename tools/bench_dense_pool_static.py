# coding=utf-8
"""One whole training step of examples/demo_diff_pool.py (two DiffPool levels of 20 and 5 clusters; feature GNN 2 x GCN(128),
assignment GNN GCN(128) -> GCN(K); mean || max readouts, Dropout -> Dense, Adam) on its dataset (graphs of 10-50 nodes,
F = 37), batches of 128 and 512 graphs, three ways:

  (A) collate   : GraphStore.collate of host-drawn ids + DiffPool.call (plans by sorting, torch.nonzero and a count read back)
  (B) static    : StaticLoader.next_ids + collate_static + DiffPool.pool_static, issued launch by launch
  (C) replayed  : (B) recorded once by tfg.CapturedTrainStep and replayed from one hipGraph

and the pooled-edge assembly alone: the three launches of tfgx_dense_pool_static (edge list, both plans, node tables) against
nn.pool.diff_pool._pooled_edges (torch.nonzero, one plan, a count read back) on the same S^T A S of level 1, both ending in a
device synchronise.

Method (that of tools/bench_sag_pool_static.py): a host clock around work that ends in a device synchronise; the variants
alternate step by step in one process, after a warm-up; the whole comparison is repeated (--repeats) so the spread between the
repeats' medians is known.  A static route counts as ahead of (A) only when its median is below (A)'s by more than the SUM of
the two spreads.  Each variant trains a model of its own.  Not measured: where inside a step the time goes (no kernel trace),
and the cost of the padded rows by itself — only their share, n_cap / live rows and e_cap / live edges per level, read from the
batches' `counts`.

    python tools/bench_dense_pool_static.py [--out profiles/dense_pool_static_bench.json]
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

# tfgx_dense_pool_static: count, scan, emit; the products, the gathers and the GNNs are not counted
LAUNCHES_PER_LEVEL = {"count": 1, "scan": 1, "emit": 1}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--batch-sizes", type=int, nargs="+", default=[128, 512])
    p.add_argument("--steps", type=int, default=50, help="timed steps per variant and repeat (at least 50)")
    p.add_argument("--warmup", type=int, default=6)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd.nn.pool.dense_pool_static import dense_pool_layout
    from tf_geometric_amd.nn.pool.diff_pool import _pooled_edges
    from demo_diff_pool import CachedGcnStack, DensePoolModel, NUM_CLUSTERS, static_loss
    from demo_sag_pool_h import graph_store, make_dataset
    assert torch.cuda.is_available(), "bench_dense_pool_static needs a GPU: there is nothing to time without one"

    data = make_dataset(args.graphs, 0)
    store = graph_store(data, range(len(data.graphs)))
    F, G = store.num_features, len(store)
    rng = np.random.Generator(np.random.PCG64(7))
    loss_static = static_loss(False)

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

    def collate_loss(model, b):
        logits = model([b.x, b.edge_index, b.node_graph_index, b.num_graphs], training=True)
        return torch.nn.functional.cross_entropy(logits, b.y.reshape(-1))

    def eager_step(opt, loss_fn):
        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn()
            loss.backward()
            opt.step()
            return loss
        return step

    def levels_of(model, batch):
        out, h = [], batch.x
        with torch.no_grad():
            for pool in model.pools:
                batch = pool.pool_static(h, batch, training=False)
                h = batch.x
                out.append(batch)
        return out

    result = {"dataset": {"graphs": G, "nodes": int(store.node_ptr[-1]), "edges": int(store.edge_ptr[-1]), "F": F},
              "clusters": list(NUM_CLUSTERS),
              "method": "host clock around work ending in a device synchronise; variants alternate step by step; ms",
              "launches_per_pooled_layout": dict(LAUNCHES_PER_LEVEL, total=sum(LAUNCHES_PER_LEVEL.values())), "batch_sizes": {}}
    for bs in args.batch_sizes:
        cap = store.static_capacities(bs)
        torch.manual_seed(0)
        pool = [rng.choice(G, bs, replace=False) for _ in range(256)]       # drawn ahead, as `batches` draws its epoch order ahead
        turn = iter(range(1 << 30))

        def host_ids():
            return pool[next(turn) % len(pool)]

        model_a = DensePoolModel(tfg.layers.DiffPool, F, 2, seed=0)
        model_b, model_c = (DensePoolModel(tfg.layers.DiffPool, F, 2, seed=0, stack=CachedGcnStack) for _ in range(2))
        loader_b = store.static_loader(bs, shuffle=True, seed=1)
        loader_c = store.static_loader(bs, shuffle=True, seed=1)
        steps = {"collate": eager_step(torch.optim.Adam(model_a.parameters(), lr=1e-3),
                                       lambda: collate_loss(model_a, store.collate(host_ids()))),
                 "static": eager_step(torch.optim.Adam(model_b.parameters(), lr=1e-3),
                                      lambda: loss_static(model_b, store.collate_static(loader_b.next_ids(), cap))),
                 "replayed": tfg.CapturedTrainStep(lambda: loss_static(model_c, store.collate_static(loader_c.next_ids(), cap)),
                                                   torch.optim.Adam(model_c.parameters(), lr=1e-3, capturable=True))}
        # the pooled-edge assembly alone, on the S^T A S of level 1 of one batch: its live slots' blocks for _pooled_edges
        batch = store.collate_static(loader_b.next_ids(), cap)
        K = NUM_CLUSTERS[0]
        level1 = levels_of(model_b, batch)[0]
        live = int(batch.counts[0])
        P = torch.zeros((bs * K * K,), device=batch.x.device)
        src = level1.edge_src[:int(level1.counts[2])].long()
        P[src] = level1.edge_weight.detach()[:src.shape[0]]
        P = P.reshape(bs * K, K)
        P_live = P[:live * K].contiguous()                                   # full batches: the live slots come first
        pcap = batch.dense_pooled_capacities(K)
        alone = {"pooled_edges_nonzero": lambda: _pooled_edges(P_live, live, K, False),
                 "static_layout": lambda: dense_pool_layout(P, batch, K, False, pcap)}
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
        for k in ("static", "replayed"):
            gap = s["median_ms"]["collate"] - s["median_ms"][k]
            entry[k + "_ahead_of_collate_beyond_spreads"] = bool(gap > s["spread_ms"]["collate"] + s["spread_ms"][k])
        # the share of padding per level, from the batches' own counts (one epoch of full batches)
        loader_b.cursor.zero_()
        per_level, levels = [], []
        for _ in range(loader_b.steps_per_epoch):
            b = store.collate_static(loader_b.next_ids(), cap)
            levels = levels_of(model_b, b)
            per_level.append(torch.stack([b.counts] + [lv.counts for lv in levels]))
        counts = torch.stack(per_level).cpu().numpy().astype(np.float64)          # [steps, 3 batches, 4]
        full = counts[:, 0, 0] == bs
        assert not counts[:, :, 3].any(), "a flag was raised"
        caps = [cap] + [lv.capacities for lv in levels]
        entry["padding"] = [{"level": i, "n_cap": c.n_cap, "e_cap": c.e_cap, "mean_live_nodes": float(counts[full, i, 1].mean()),
                             "mean_live_edges": float(counts[full, i, 2].mean()),
                             "n_cap_over_live": float(c.n_cap / counts[full, i, 1].mean()),
                             "e_cap_over_live": float(c.e_cap / max(counts[full, i, 2].mean(), 1.0))} for i, c in enumerate(caps)]
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: step  collate {:.3f}  static {:.3f}  replayed {:.3f} ms  (spreads {:.3f} / {:.3f} / {:.3f})  "
              "ahead of collate beyond spreads: static {}  replayed {}".format(
                  bs, *(s["median_ms"][k] for k in steps), *(s["spread_ms"][k] for k in steps),
                  entry["static_ahead_of_collate_beyond_spreads"], entry["replayed_ahead_of_collate_beyond_spreads"]), flush=True)
        a = entry["assembly_alone"]
        print("            assembly alone: _pooled_edges {:.3f}  static layout {:.3f} ms  (spreads {:.3f} / {:.3f})".format(
            a["median_ms"]["pooled_edges_nonzero"], a["median_ms"]["static_layout"], a["spread_ms"]["pooled_edges_nonzero"],
            a["spread_ms"]["static_layout"]), flush=True)
        for lv in entry["padding"]:
            print("            level {level}: n_cap {n_cap} / live {mean_live_nodes:.0f} = {n_cap_over_live:.2f}   "
                  "e_cap {e_cap} / live {mean_live_edges:.0f} = {e_cap_over_live:.2f}".format(**lv), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
