# coding=utf-8
"""One whole training step of examples/demo_sag_pool_h.py (3 x (GCN(128) -> SAGPool(GCN(1), ratio 0.5, tanh)), mean || max
readouts, a 3-layer MLP, Adam) on its dataset (4000 graphs of 10-50 nodes, F = 37), batches of 128 and 512 graphs, three ways:

  (A) collate        : GraphStore.collate of host-drawn ids + SAGPool.call (topk_pool, induced_subgraph: host reads and sorts)
  (B) static         : StaticLoader.next_ids + collate_static + SAGPool.pool_static, issued launch by launch
  (C) replayed       : (B) recorded once by tfg.CapturedTrainStep and replayed from one hipGraph

and the selection alone: tfgx_static_pool_table + tfgx_static_pool_select against tfgx_segment_topk on the same batch and scores,
both ending in a device synchronise (topk_pool also reads its count back; that read is part of what it costs); and the mean +
max readouts of the three pooled levels, forward only, over the padded static batches against the live rows alone.

Method (that of tools/bench_collate_static.py): a host clock around work that ends in a device synchronise; the variants
alternate step by step in one process, after a warm-up; the whole comparison is repeated (--repeats) so the spread between the
repeats' medians is known.  (C) counts as ahead of (A) only when its median is below (A)'s by more than the SUM of the two
spreads.  Each variant trains a model of its own.  Launches per pooling level are counted from the code, not traced.  Not
measured: where inside a step the time goes (no kernel trace), and the cost of the padded rows by itself — only their share,
n_cap' / m_live and e_cap / e_kept per level, read from the batches' `counts`.

    python tools/bench_sag_pool_static.py [--out profiles/sag_pool_static_bench.json]
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

# tfgx_static_pool_table, _select, _edges (count, scan, emit edges, emit plans), _gather_scale_rows_f32; the score GCN not counted
LAUNCHES_PER_LEVEL = {"table": 1, "select": 1, "edges": 4, "features": 1}


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
    from demo_sag_pool_h import SAGPoolHModel, graph_store, make_dataset, static_logits, static_loss
    assert torch.cuda.is_available(), "bench_sag_pool_static needs a GPU: there is nothing to time without one"

    data = make_dataset(args.graphs, 0)
    store = graph_store(data, range(len(data.graphs)))
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

    result = {"dataset": {"graphs": G, "nodes": int(store.node_ptr[-1]), "edges": int(store.edge_ptr[-1]), "F": F},
              "method": "host clock around work ending in a device synchronise; variants alternate step by step; ms",
              "launches_per_pooling_level": dict(LAUNCHES_PER_LEVEL, total=sum(LAUNCHES_PER_LEVEL.values())), "batch_sizes": {}}
    for bs in args.batch_sizes:
        cap = store.static_capacities(bs)
        torch.manual_seed(0)
        pool = [rng.choice(G, bs, replace=False) for _ in range(256)]       # drawn ahead, as `batches` draws its epoch order ahead
        turn = iter(range(1 << 30))

        def host_ids():
            return pool[next(turn) % len(pool)]

        model_a, model_b, model_c = (SAGPoolHModel(F, 2, seed=0) for _ in range(3))
        loader_b = store.static_loader(bs, shuffle=True, seed=1)
        loader_c = store.static_loader(bs, shuffle=True, seed=1)
        steps = {"collate": eager_step(torch.optim.Adam(model_a.parameters(), lr=5e-4),
                                       lambda: collate_loss(model_a, store.collate(host_ids()))),
                 "static": eager_step(torch.optim.Adam(model_b.parameters(), lr=5e-4),
                                      lambda: static_loss(model_b, store.collate_static(loader_b.next_ids(), cap))),
                 "replayed": tfg.CapturedTrainStep(lambda: static_loss(model_c, store.collate_static(loader_c.next_ids(), cap)),
                                                   torch.optim.Adam(model_c.parameters(), lr=5e-4, capturable=True))}
        # the selection alone, on one batch and the scores of a GCN(1)-shaped vector
        batch = store.collate_static(loader_b.next_ids(), cap)
        n_live = int(batch.counts[1])
        score = torch.randn(cap.n_cap, device=batch.x.device)
        ngi_live, score_live = batch.node_graph_index[:n_live].contiguous(), score[:n_live].contiguous()
        alone = {"segment_topk": lambda: tfg.nn.topk_pool(ngi_live, score_live, ratio=0.5, num_segments=bs),
                 "static_select": lambda: tfg.nn.topk_pool_static(batch, score, ratio=0.5)}
        # what the padded rows cost in the readouts: mean + max of the three pooled levels of that batch, forward only, through the
        # plans the static batches carry (the dead graph B is one row of n_cap' - m_live nodes, walked by one lane group:
        # DESIGN.md 2.26) against the same readouts over the live rows alone (a cached plan of their own, no sort in the loop)
        levels = []
        with torch.no_grad():
            static_logits(model_b, batch, training=False, levels=levels)
        live = []
        for lv in levels:
            m = int(lv.counts[1])
            live.append((lv.x.detach()[:m].contiguous(), lv.node_graph_index[:m].contiguous(), {}))
        readouts = {"static_padded": lambda: [lv.readout(lv.x.detach(), op) for lv in levels for op in ("mean", "max")],
                    "live_rows_only": lambda: [getattr(tfg.nn, op + "_pool")(x, g, bs, cache=c) for x, g, c in live
                                               for op in ("mean", "max")]}
        entry = {"capacities": cap._asdict()}
        for what, variants in (("step", steps), ("selection_alone", alone), ("readouts_forward", readouts)):
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
        # the share of padding per level, from the batches' own counts (one epoch of full batches)
        loader_b.cursor.zero_()
        per_level = []
        with torch.no_grad():
            for _ in range(loader_b.steps_per_epoch):
                b = store.collate_static(loader_b.next_ids(), cap)
                levels = []
                static_logits(model_b, b, training=False, levels=levels)
                per_level.append(torch.stack([b.counts] + [lv.counts for lv in levels]))
        counts = torch.stack(per_level).cpu().numpy().astype(np.float64)          # [steps, 4 batches, 4]
        full = counts[:, 0, 0] == bs
        assert not counts[:, :, 3].any(), "a flag was raised"
        caps = [cap]
        for lv in levels:
            caps.append(lv.capacities)
        entry["padding"] = [{"level": i, "n_cap": c.n_cap, "e_cap": c.e_cap, "mean_live_nodes": float(counts[full, i, 1].mean()),
                             "mean_live_edges": float(counts[full, i, 2].mean()),
                             "n_cap_over_live": float(c.n_cap / counts[full, i, 1].mean()),
                             "e_cap_over_live": float(c.e_cap / max(counts[full, i, 2].mean(), 1.0))} for i, c in enumerate(caps)]
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: step  collate {:.3f}  static {:.3f}  replayed {:.3f} ms  (spreads {:.3f} / {:.3f} / {:.3f})  "
              "replayed ahead beyond spreads: {}".format(bs, *(s["median_ms"][k] for k in steps), *(s["spread_ms"][k] for k in steps),
                                                         entry["replayed_ahead_of_collate_beyond_spreads"]), flush=True)
        a = entry["selection_alone"]
        print("            selection alone: segment_topk {:.3f}  static table + select {:.3f} ms  (spreads {:.3f} / {:.3f})".format(
            a["median_ms"]["segment_topk"], a["median_ms"]["static_select"], a["spread_ms"]["segment_topk"],
            a["spread_ms"]["static_select"]), flush=True)
        r = entry["readouts_forward"]
        print("            mean + max readouts of the 3 levels, forward: static (padded) {:.3f}  live rows only {:.3f} ms  "
              "(spreads {:.3f} / {:.3f})".format(r["median_ms"]["static_padded"], r["median_ms"]["live_rows_only"],
                                                 r["spread_ms"]["static_padded"], r["spread_ms"]["live_rows_only"]), flush=True)
        for lv in entry["padding"]:
            print("            level {level}: n_cap {n_cap} / live {mean_live_nodes:.0f} = {n_cap_over_live:.2f}   "
                  "e_cap {e_cap} / live {mean_live_edges:.0f} = {e_cap_over_live:.2f}".format(**lv), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
