# coding=utf-8
"""One whole training step of examples/demo_asap.py (3 x (GCN(64) -> ASAP(ratio 0.5, drop 0.1)), mean || max readouts, a 2-layer
MLP, Adam) on its dataset (4000 graphs of 10-50 nodes, F = 37), batches of 128 and 512 graphs, three ways:

  (A) collate        : GraphStore.collate of host-drawn ids + ASAP.call (host reads, a sort per call, the sparse S^T A S)
  (B) static         : StaticLoader.next_ids + collate_static + ASAP.pool_static, issued launch by launch
  (C) replayed       : (B) recorded once by tfg.CapturedTrainStep and replayed from one hipGraph

and the new pieces alone on one batch's first level: the attention with absent edges (tfgx_asapstatic_attend_f32), the dense
assignment (tfgx_asapstatic_assign_f32), the pooled edges with both plans (tfgx_asapstatic_edges: count, scan, emit), and the
centred attention backward (tfgx_asapstatic_attend_backward_f32) beside the entry nn.asap uses (tfgx_asap_attend_backward_f32)
on the same inputs; and the share of padding, n_cap / live rows and e_cap / live edges per level, read
from the batches' `counts`.

Method (that of tools/bench_sag_pool_static.py): a host clock around work that ends in a device synchronise; the variants
alternate step by step in one process, after a warm-up; the whole comparison is repeated (--repeats) so the spread between the
repeats' medians is known.  (C) counts as ahead of (A) only when its median is below (A)'s by more than the SUM of the two
spreads.  Each variant trains a model of its own.  Launches per pooling level are counted from the code, not traced.  Not
measured: where inside a step the time goes (no kernel trace), and the cost of the padded rows by itself.

    python tools/bench_asap_static.py [--out profiles/asap_static_bench.json]
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

# the level's own device code (nn/pool/asap_static.py): tfgx_asapstatic_attend_f32; tfgx_static_pool_table, _select;
# tfgx_static_pool_gather_scale_rows_f32; tfgx_asapstatic_assign_f32 (zero S, scatter); A1 S (tfgx_segment_reduce_f32);
# tfgx_segment_gram_f32 (2); tfgx_asapstatic_edges (count, scan, emit).  The GCN, the max aggregation, LEConv and the small GEMMs
# that ASAP.call launches as well are not counted.
LAUNCHES_PER_LEVEL = {"attention": 1, "table": 1, "select": 1, "features": 1, "assignment": 2, "A1_S": 1, "gram": 2, "edges": 3}


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
    from tf_geometric_amd import autograd as AG
    from tf_geometric_amd.plan import CACHE_KEY_PLAN
    from tf_geometric_amd.nn.pool.asap_static import asap_assignment, asap_layout
    from tf_geometric_amd.nn.pool.sag_pool_static import select_static
    from demo_asap import ASAPModel, static_loss
    from demo_sag_pool_h import graph_store, make_dataset
    assert torch.cuda.is_available(), "bench_asap_static needs a GPU: there is nothing to time without one"

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

        model_a, model_b, model_c = (ASAPModel(F, 2, seed=0) for _ in range(3))
        loader_b = store.static_loader(bs, shuffle=True, seed=1)
        loader_c = store.static_loader(bs, shuffle=True, seed=1)
        steps = {"collate": eager_step(torch.optim.Adam(model_a.parameters(), lr=5e-4),
                                       lambda: collate_loss(model_a, store.collate(host_ids()))),
                 "static": eager_step(torch.optim.Adam(model_b.parameters(), lr=5e-4),
                                      lambda: static_loss(model_b, store.collate_static(loader_b.next_ids(), cap))),
                 "replayed": tfg.CapturedTrainStep(lambda: static_loss(model_c, store.collate_static(loader_c.next_ids(), cap)),
                                                   torch.optim.Adam(model_c.parameters(), lr=5e-4, capturable=True))}
        # the three new pieces alone, on the first level of one batch: random scores of the shapes the level makes
        batch = store.collate_static(loader_b.next_ids(), cap)
        plan = batch.cache[CACHE_KEY_PLAN]
        dev = batch.x.device
        x = torch.randn(cap.n_cap, 64, device=dev)
        sq, sh, bias = torch.randn(cap.n_cap, device=dev), torch.randn(cap.n_cap, device=dev), torch.zeros(1, device=dev)
        pcap = batch.asap_pooled_capacities(ratio=0.5)
        K = batch.asap_clusters_per_graph(ratio=0.5)
        sel = select_static(batch, sq, None, 0.5, pcap, "bench")
        _, pw, pws, _, _ = AG.asap_attend_forward(plan, x, sq, sh, bias, skip_self_loops=True)
        S = asap_assignment(plan, pw, pws, sel, bs, K)
        P = torch.rand(bs * K, K, device=dev) * (torch.rand(bs * K, K, device=dev) < 0.3)
        _, p, ps, _, _ = AG.asap_attend_forward(plan, x, sq, sh, bias, skip_self_loops=True)
        dp, dps = torch.randn(cap.e_cap, device=dev), torch.randn(cap.n_cap, device=dev)
        ds, dss, dsq = torch.empty(cap.e_cap, device=dev), torch.empty(cap.n_cap, device=dev), torch.empty(cap.n_cap, device=dev)
        L, lib = tfg._lib, tfg._lib.require_gpu()
        head = [L.ptr(plan.row_ptr), L.ptr(plan.col), cap.n_cap, cap.e_cap, L.ptr(sq), L.ptr(sh), L.ptr(bias), L.ptr(p), L.ptr(ps), None,
                None, L.ptr(dp), L.ptr(dps)]
        tail = [L.ptr(ds), L.ptr(dss), L.ptr(dsq)]
        alone = {"attention": lambda: AG.asap_attend_forward(plan, x, sq, sh, bias, skip_self_loops=True),
                 "assignment": lambda: asap_assignment(plan, pw, pws, sel, bs, K),
                 "edges_and_plans": lambda: asap_layout(P, sel.pooled_row_ptr, sel.counts, K, pcap),
                 "attention_backward_centred": lambda: L.check(lib.tfgx_asapstatic_attend_backward_f32(*head, 1, *tail, L.stream_ptr())),
                 "attention_backward_of_nn_asap": lambda: L.check(lib.tfgx_asap_attend_backward_f32(*head, *tail, L.stream_ptr()))}
        del S
        entry = {"capacities": cap._asdict(), "clusters_per_graph_level_1": K}
        for what, variants in (("step", steps), ("new_pieces_alone_level_1", alone)):
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
                model_b.static(b, training=False, levels=levels)
                per_level.append(torch.stack([b.counts] + [lv.counts for lv in levels]))
        counts = torch.stack(per_level).cpu().numpy().astype(np.float64)          # [steps, 4 batches, 4]
        full = counts[:, 0, 0] == bs
        assert not counts[:, :, 3].any(), "a flag was raised"
        caps = [cap] + [lv.capacities for lv in levels]
        entry["padding"] = [{"level": i, "n_cap": c.n_cap, "e_cap": c.e_cap, "mean_live_nodes": float(counts[full, i, 1].mean()),
                             "mean_live_edges": float(counts[full, i, 2].mean()),
                             "n_cap_over_live": float(c.n_cap / counts[full, i, 1].mean()),
                             "e_cap_over_live": float(c.e_cap / max(counts[full, i, 2].mean(), 1.0))} for i, c in enumerate(caps)]
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: step  collate {:.3f}  static {:.3f}  replayed {:.3f} ms  (spreads {:.3f} / {:.3f} / {:.3f})  "
              "replayed ahead beyond spreads: {}".format(bs, *(s["median_ms"][k] for k in steps), *(s["spread_ms"][k] for k in steps),
                                                         entry["replayed_ahead_of_collate_beyond_spreads"]), flush=True)
        a = entry["new_pieces_alone_level_1"]
        print("            alone, level 1: attention {:.3f}  assignment {:.3f}  edges + plans {:.3f}  backward centred {:.3f}  "
              "backward of nn.asap {:.3f} ms".format(*(a["median_ms"][k] for k in alone)), flush=True)
        for lv in entry["padding"]:
            print("            level {level}: n_cap {n_cap} / live {mean_live_nodes:.0f} = {n_cap_over_live:.2f}   "
                  "e_cap {e_cap} / live {mean_live_edges:.0f} = {e_cap_over_live:.2f}".format(**lv), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
